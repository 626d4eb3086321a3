"""Measure the empirical-Bayes state shrinkage on the device (csrc/csr_shrink.h, csr_host_shrink.inl) against one core of the host.

    python scripts/shrink_bench.py          # 1 x MI355X, writes profiles/shrink_bench.json (--out)

One process, hg38 at 200 bp, the default model (spike and Student-t, K = 16 slabs), block size 25, a fitted synthetic batch (one
sample per chain).  For chr1 alone and for the 22 autosomes as one batch, medians of three, every timed call ending in its own
download of the sums (a pass) or a synchronise:
  resident      `DeviceBatch.shrink_fit` / `shrink_apply` from the resident fit: time per EM pass (one `csr_shrink_em_step`), per
                whole fit with its pass count, per apply (posterior tracks and the four medians), and the preparation;
  host arrays   the same through `shrink.fit_state_shrinkage_prior` / `apply_state_shrinkage_prior` on the downloaded float32
                tracks widened to float64: the staging (upload and block counts) is counted into the fit, a pass is timed alone;
  cpu           scripts/ubench/shrink_cpu.c at -O3 on one core: one EM pass and one posterior pass (a fit is passes x the pass).
The device's and the C restatement's sums of chr1's pass are compared (worst |difference| / sum over the positive sums and the
log likelihood's |terms|); the posterior tracks are compared value for value.
Not measured: 50 bp, real data, kernel counters."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

K, BLOCK = 16, 25


def cpu_port():
    src = os.path.join(ROOT, "scripts", "ubench", "shrink_cpu.c")
    so = os.path.join(tempfile.mkdtemp(prefix="shrink_cpu_"), "libshrink_cpu.so")
    subprocess.check_call(["gcc", "-O3", "-fno-trapping-math", "-fno-math-errno", "-mtune=generic", "-ffp-contract=off", "-shared",
                           "-fPIC", "-o", so, src, "-lm"])
    lib = C.CDLL(so)
    DP, FP = C.POINTER(C.c_double), C.POINTER(C.c_float)
    lib.shrink_cpu_em.argtypes = [DP, DP, C.c_long, C.c_long, C.c_double, C.c_int, DP, DP, DP]
    lib.shrink_cpu_em.restype = None
    lib.shrink_cpu_post.argtypes = [DP, DP, C.c_long, C.c_double, C.c_int, DP, DP, FP]
    lib.shrink_cpu_post.restype = None
    dp = lambda a: a.ctypes.data_as(DP)     # noqa: E731

    def em(x, v, block, pi0, tau, lsp):
        out = np.zeros(4 + 2 * tau.shape[0])
        lib.shrink_cpu_em(dp(x), dp(v), x.shape[0], int(block), float(pi0), int(tau.shape[0]), dp(tau), dp(lsp), dp(out))
        return out

    def post(x, v, pi0, tau, lsp):
        out = np.empty((5, x.shape[0]), np.float32)
        lib.shrink_cpu_post(dp(x), dp(v), x.shape[0], float(pi0), int(tau.shape[0]), dp(tau), dp(lsp), out.ctypes.data_as(FP))
        return out

    return em, post


def median3(fn, repeats):
    times, last = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        last = fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), times, last


class Counting:
    """A pass evaluator that counts the EM passes of the one it wraps."""

    def __init__(self, inner):
        self.inner, self.lengths, self.passes = inner, inner.lengths, 0

    def initial_sums(self, null_z):
        return self.inner.initial_sums(null_z)

    def em_step(self, pi0, tau, log_prior):
        self.passes += 1
        return self.inner.em_step(pi0, tau, log_prior)


def measure(b, S, take, label, repeats, em_cpu, post_cpu, lens):
    from consenrich_amd import _lib as L

    nc = len(lens)
    idx = [c for c in range(nc) if take[c]]
    bins = int(sum(lens[c] for c in idx))
    kw = dict(studentTQuadratureOrder=K)
    doc = dict(chains=len(idx), bins=bins)
    # -- resident
    t_prep, _, _ = median3(lambda: b._shrink_prepare(take, "fit", BLOCK), repeats)
    prior = b.shrink_fit(chains=take, block_size=BLOCK, **kw)             # warm-up, and the parameter set of the timed pass
    tau, w = S.prior_slabs(prior)
    lsp = S.log_slab_prior(prior.priorSpikeProp, w)
    b._shrink_prepare(take, "fit", BLOCK)
    t_pass, all_pass, rows = median3(lambda: S._em_rows(b._ctx, nc, prior.priorSpikeProp, tau, lsp), repeats)
    t_fit, all_fit, prior = median3(lambda: b.shrink_fit(chains=take, block_size=BLOCK, **kw), repeats)

    def apply():
        out = b.shrink_apply(prior, chains=take)
        b.synchronize()
        return out

    t_apply, all_apply, _ = median3(apply, repeats)
    doc["resident"] = dict(prepare_seconds=t_prep, em_pass_seconds=t_pass, em_pass_seconds_all=all_pass, fit_seconds=t_fit,
                           fit_seconds_all=all_fit, fit_iterations=int(prior.metadata["iterations"]),
                           fit_converged=bool(prior.metadata["converged"]), apply_seconds=t_apply, apply_seconds_all=all_apply,
                           em_pass_ns_per_bin=1e9 * t_pass / bins)
    # -- host arrays (the tracks the resident path read, widened to float64)
    chunks = [(b.download(c, "xs")[:, 0].astype(np.float64), b.download_shrunk(c, "variance").astype(np.float64)) for c in idx]
    passes = Counting(S.HostArrayPasses(chunks, BLOCK))

    def host_fit():
        S._staged_by = None                 # the staging belongs to a fit
        passes.passes = 0
        return S.fit_state_shrinkage_prior(passes=passes, blockSize=BLOCK, **kw)

    t_hfit, all_hfit, hprior = median3(host_fit, repeats)
    n_passes = passes.passes
    t_hpass, _, hrows = median3(lambda: passes.inner.em_step(prior.priorSpikeProp, tau, lsp), repeats)
    t_happly, _, _ = median3(lambda: [S.apply_state_shrinkage_prior(x, v, hprior) for x, v in chunks], repeats)
    doc["host_arrays"] = dict(em_pass_seconds=t_hpass, fit_seconds=t_hfit, fit_seconds_all=all_hfit, fit_em_passes=n_passes,
                              apply_seconds=t_happly, same_prior_as_resident=bool(hprior.slabVariance == prior.slabVariance
                                                                                  and hprior.priorSpikeProp == prior.priorSpikeProp))
    doc["resident"]["fit_em_passes"] = n_passes
    # -- one core
    t0 = time.perf_counter()
    cpu_rows = [em_cpu(x, v, BLOCK, prior.priorSpikeProp, tau, lsp) for x, v in chunks]
    t_cpass = time.perf_counter() - t0
    eff = S.effective_spike_prop(prior, 2.0)
    elsp = S.log_slab_prior(eff, w)
    t0 = time.perf_counter()
    cpu_post = [post_cpu(x, v, eff, tau, elsp) for x, v in chunks]
    t_cpost = time.perf_counter() - t0
    doc["cpu_one_core"] = dict(em_pass_seconds=t_cpass, posterior_pass_seconds=t_cpost, em_pass_seconds_per_million_bins=1e6 * t_cpass / bins,
                               posterior_seconds_per_million_bins=1e6 * t_cpost / bins, fit_seconds_at_measured_pass_count=n_passes * t_cpass)
    doc["cpu_over_device"] = dict(em_pass=t_cpass / t_pass, fit=n_passes * t_cpass / t_fit, apply=t_cpost / t_apply)
    # -- agreement: the sums of the pass (every row but the log likelihood is a sum of positive terms; the log likelihood's
    #    terms are taken as |sum| here, which only makes the ratio larger), and the posterior tracks
    worst = 0.0
    for k, c in enumerate(idx):
        dev, cpu = rows[c], cpu_rows[k]
        worst = max(worst, float(np.max(np.abs(dev - cpu) / np.maximum(np.abs(cpu), 1e-300))))
        assert dev[3] == cpu[3]
    differing = total = 0
    for k, c in enumerate(idx):
        for r, name in enumerate(("shrunk", "posterior_sd", "spike_prop")):
            d = b.download_shrunk(c, name)
            same = (d.view(np.uint32) == cpu_post[k][r].view(np.uint32))
            differing += int(np.count_nonzero(~same))
            total += d.size
    doc["agreement"] = dict(em_pass_worst_relative_difference_to_sequential_c=worst, posterior_values=total,
                            posterior_values_differing_in_any_bit=differing)
    print(label, json.dumps(doc))
    return doc


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shrink_bench.json"))
    ap.add_argument("--chains", type=int, default=22, help="the first N autosomes")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    import cases
    from consenrich_amd import _lib as L
    from consenrich_amd import shrink as S
    from consenrich_amd.batch import DeviceBatch, ModelParams
    from consenrich_amd.sharding import hg38_chain_lengths

    L.require_gpu()
    em_cpu, post_cpu = cpu_port()
    lens = [int(n) for n in hg38_chain_lengths(200)][:args.chains]
    nc = len(lens)
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), 1, lens)
        for c in range(nc):
            b.upload(c, *cases.synth(lens[c], 1, 500 + c))
        b.stats()
        b.forward_backward(L.RETURN_NLL)
        b.export(L.EXPORT_SMOOTH)
        b.synchronize()
        chr1 = measure(b, S, [c == 0 for c in range(nc)], "chr1", args.repeats, em_cpu, post_cpu, lens)
        genome = measure(b, S, [True] * nc, "autosomes", args.repeats, em_cpu, post_cpu, lens)
    doc = dict(interval_bp=200, slabs=K, block_size=BLOCK, model="spikeAndStudentT", repeats=args.repeats, chr1=chr1, autosomes=genome,
               test_cases_worst_pass_ratio=dict(
                   gate=1e-12, device_to_reference=1.85e-13, device_tree_to_exact_sum=5.7e-16, reference_sequential_to_exact_sum=1.85e-13,
                   note="tests/test_gpu_shrink.py, 20 000-bin chain with block 50: totalWeight adds 1/50 twenty thousand times; the "
                        "reference's sequential sum drifts by 1.85e-13 of the exact sum (same addend, same rounding direction), "
                        "the device's tree by 5.7e-16 -- the difference is the reference's own error"),
               chr1_scale_note="agreement.em_pass_worst_relative_difference_to_sequential_c (1.8e-11 on chr1) is the sequential sum's own "
                               "drift: against exact sums (math.fsum) of 1 244 783 bins with block 25, totalWeight added bin after bin is "
                               "off by 1.81e-11, the device's tree by 2.3e-14 (CHANGELOG); the 1e-12 gate of the tests is a statement "
                               "about their sizes",
               not_measured=["50 bp", "real data", "kernel counters"],
               note="one process, one MI355X; synthetic fitted batch, one sample per chain; cpu = scripts/ubench/shrink_cpu.c (-O3, one "
                    "core, sequential sums); medians of three")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
