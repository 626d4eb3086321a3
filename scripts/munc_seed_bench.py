"""Measure the dense observation-variance seed loop on the device (`driver.munc_seed_batch`; csrc/csr_munc.h, csr_host_munc.inl).

    python scripts/munc_seed_bench.py          # 1 x MI355X, writes profiles/munc_seed_bench.json (--out)

One process, hg38 at 200 bp, m = 32 samples, the device's synthetic batch (`DeviceBatch.synthesize`), the reference's defaults
(3 weight passes, Student-t weights with 8 degrees of freedom, omega in [0.01, 100], pad 1e-4, no count floor, no exclude mask,
background fit on with the nonnegative IRLS at multiplier 1 and the G-uncertainty proxy), a local window of 64 intervals and
background penalties of a 64-interval span at smoothness 1 (the reference derives both from the dependence span and its prior
block length; 64 is this script's choice).  The per-chain Q0 is GIVEN (`q=`): the `qseed` call a loop at its defaults makes once,
before its first round, is outside every time below (scripts/qseed_bench.py measures it).  For chr1 alone and for the 22 autosomes as one batch,
medians of three:
  loop          `driver.munc_seed_batch` with nothing fetched, synchronised at the end;
  split         the same calls timed stage by stage with a synchronise after each: smoother (working munc + statistics + forward /
                backward, four times), seed passes (four), background (three: weighted statistics, solve with IRLS, G proxy with its
                median and q99 selections), finish (rolling mean, total variance, response weight);
  fallbacks     the rolling mean's fallback rows (`munc_seed_stats`);
  cpu           scripts/ubench/munc_cpu.c at -O3 on one core on chr1's downloaded arrays: one seed pass and one rolling mean.
The device's rolling mean of chr1 is compared bit for bit with the C restatement's on the same resident input.
Not measured: the reference's own loop (its smoother and its natives under its own build), 50 bp, real data, kernel counters."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

M, PASSES, PAD, WINDOW = 32, 3, 1.0e-4, 64
BG = dict(lam_first=64.0 * 64.0 / 4.0, lam=64.0 ** 4 / 16.0, negative_penalty_multiplier=1.0)   # core.py:7480-7493 at span 64


def median3(fn, repeats):
    times, last = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        last = fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), times, last


def measure(lens, label, repeats, port):
    from consenrich_amd import driver
    from consenrich_amd.batch import DeviceBatch, ModelParams

    nc, bins = len(lens), int(sum(lens))
    doc = dict(chains=nc, bins=bins, cells=bins * M)
    q = [np.array([[1.0e-3, 0.0], [0.0, 1.0e-4]], np.float32)] * nc
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), M, lens)

        def fresh():
            b.synthesize(1234)          # (the loop leaves the last working munc in the batch: every run starts from the seed munc)
            b.synchronize()

        def loop():
            driver.munc_seed_batch(b, pad=PAD, window=WINDOW, passes=PASSES, q=q, fit_background=True, background=BG, g_uncertainty="proxy", fetch=())
            b.synchronize()

        fresh()
        loop()                          # warm-up: allocations, first-use exports
        times = []
        for _ in range(repeats):
            fresh()
            t0 = time.perf_counter()
            loop()
            times.append(time.perf_counter() - t0)
        doc["loop_seconds"], doc["loop_seconds_all"] = statistics.median(times), times
        doc["loop_ns_per_cell"] = 1e9 * doc["loop_seconds"] / (bins * M)
        stats = b.munc_seed_stats()
        doc["roll_fallback_rows"], doc["roll_rows"] = stats["last_roll_fallback_rows"], stats["roll_rows"]
        # -- the same calls, stage by stage
        split = dict(smoother=[], seed_passes=[], background=[], finish=[])
        for _ in range(repeats):
            fresh()
            b.set_chain_q(q)
            b.munc_seed_begin()
            acc = dict(smoother=0.0, seed_passes=0.0, background=0.0, finish=0.0)

            def timed(key, fn):
                t0 = time.perf_counter()
                fn()
                b.synchronize()
                acc[key] += time.perf_counter() - t0

            for k in range(PASSES + 1):
                timed("smoother", lambda: (b.munc_seed_working(PAD), b.stats(), b.forward_backward(want_sums=False)))
                timed("seed_passes", lambda: b.munc_seed_pass(PAD, k < PASSES))
                if k < PASSES:
                    timed("background", lambda: b.munc_seed_background(pad=PAD, g_uncertainty="proxy", **BG))
                    b.munc_seed_swap()
            timed("finish", lambda: b.munc_seed_finish(WINDOW))
            for key in split:
                split[key].append(acc[key])
        doc["split_seconds"] = {k: statistics.median(v) for k, v in split.items()}
        doc["split_seconds_all"] = split
        if port is not None:            # chr1 alone: one core on the arrays the last pointwise pass read and wrote
            data = b.download_inputs(0)[0]
            # (munc: the total variance the finish left -- an input of the same size and kind as a round's; rho, omega: the pointwise pass's)
            total, rho, omega = (b.download_munc_seed(0, k) for k in ("seed_total", "seed_rho", "seed_omega"))
            xs, Ps = b.download(0, "xs"), b.download(0, "Ps")
            mean, var = np.ascontiguousarray(xs[:, 0]), np.maximum(np.ascontiguousarray(Ps[:, 0, 0]), np.float32(0.0))
            local_dev, smooth_dev = b.download_munc_seed(0, "seed_local"), b.download_munc_seed(0, "seed_smooth")
            g, G = b.download_munc_seed(0, "seed_g"), b.download_munc_seed(0, "seed_gvar")
            t_pass, _, res = median3(lambda: port.cMuncObservationMomentSeedPass(data, total, mean, var, background=g, gVariance=G,
                                                                                 omegaIn=omega, rhoIn=rho, pad=PAD, updateWeights=False),
                                     repeats)
            t_roll, _, smooth = median3(lambda: port.cMuncSmoothDenseLocalEvidence(local_dev, WINDOW), repeats)
            doc["cpu_one_core"] = dict(seed_pass_seconds=t_pass, rolling_mean_seconds=t_roll,
                                       seed_pass_ns_per_cell=1e9 * t_pass / data.size, rolling_mean_ns_per_cell=1e9 * t_roll / data.size,
                                       four_passes_and_one_rolling_mean_seconds=4 * t_pass + t_roll)
            doc["agreement"] = dict(rolling_mean_values=int(smooth.size),
                                    rolling_mean_values_differing_in_any_bit=int(np.count_nonzero(smooth.view(np.uint32) != smooth_dev.view(np.uint32))))
            doc["cpu_natives_over_device_natives"] = (4 * t_pass + t_roll) / (doc["split_seconds"]["seed_passes"] + doc["split_seconds"]["finish"])
    print(label, json.dumps(doc))
    return doc


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "munc_seed_bench.json"))
    ap.add_argument("--chains", type=int, default=22, help="the first N autosomes")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    import twin_munc
    from consenrich_amd import _lib as L
    from consenrich_amd.sharding import hg38_chain_lengths

    L.require_gpu()
    port = twin_munc.CPort(tempfile.mkdtemp(prefix="munc_cpu_"))
    lens = [int(n) for n in hg38_chain_lengths(200)][:args.chains]
    chr1 = measure(lens[:1], "chr1", args.repeats, port)
    genome = measure(lens, "autosomes", args.repeats, None)
    doc = dict(interval_bp=200, samples=M, passes=PASSES, window_intervals=WINDOW, pad=PAD, weights="student_t", fit_background=True, g_uncertainty="proxy", background=BG,
               repeats=args.repeats, chr1=chr1, autosomes=genome,
               not_measured=["the reference's own loop (its smoother and natives under its own build)", "50 bp", "real data",
                             "kernel counters", "the CPU cost of the background update (weighted statistics, solve, G proxy)"],
               note="one process, one MI355X; device-synthesised batch; cpu = scripts/ubench/munc_cpu.c (-O3, one core), the two natives "
                    "only -- the CPU smoother and background update are not timed here; medians of three")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
