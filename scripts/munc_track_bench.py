"""Measure the stages between the seed loop and a finished matrixMunc on the device (`DeviceBatch.munc_block_sums`,
`munc_prior_track`, `munc_track_finish`; csrc/csr_munc_track.h, csr_host_munc_track.inl).

    python scripts/munc_track_bench.py          # 1 x MI355X, writes profiles/munc_track_bench.json (--out)

One process, hg38 at 200 bp, m = 32 samples, the device's synthetic batch (`DeviceBatch.synthesize`) after one round of the seed
loop without the background fit (`driver.munc_seed_batch`, passes=1: the stages below do not depend on how the seed arrays were
made), an exclude mask with 2 % of the intervals set, blocks of 50 intervals, a planted degree-3 trend with 60 basis functions,
Nu_L = 8, Nu_0 = 40 and replicate factors off 1 for every second sample.  For chr1 alone and for the 22 autosomes as one batch,
medians of three, every stage synchronised (each ends in a download or a host synchronise):
  resident      block sums (records downloaded), `pooled_block_rows` on the host (with SciPy's trigamma), prior track, finish;
  drop-ins      chr1 only, from host arrays: `munc_track.block_sums`, and per sample `eval_pspline_log_variance_trend` and
                `get_munc_track` with the prior track given, then `apply_blacklist_munc_floor` (uploads and downloads included);
  twin          chr1 only: the reference's block loop in NumPy (tests/twin_munc_track.py) on the first `--twin-blocks` blocks of
                the downloaded arrays, one run, and its time per (block, sample) pair times chr1's pairs as an EXTRAPOLATION.
Not measured: 50 bp, real data, the reference's own loop (its natives under its own build, its thread pool), kernel counters."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

M, PAD, WINDOW, BLOCK = 32, 1.0e-4, 64, 50
FLOOR, CAP = 1.0e-6, None
NU_L, NU_0 = 8.0, 40.0


def planted_trend():
    import munc_track_cases as MC

    return MC.make_trend(3, 60, 2024, x_min=-3.0, x_max=6.0)


def measure(lens, label, repeats, host_side, twin_blocks):
    from consenrich_amd import driver
    from consenrich_amd import munc_track as MT
    from consenrich_amd.batch import DeviceBatch, ModelParams

    nc, bins = len(lens), int(sum(lens))
    doc = dict(chains=nc, bins=bins, cells=bins * M)
    q = [np.array([[1.0e-3, 0.0], [0.0, 1.0e-4]], np.float32)] * nc
    rng = np.random.default_rng(7)
    exclude = [(rng.random(n) < 0.02).astype(np.uint8) for n in lens]
    trend = planted_trend()
    factors = [1.0 if j % 2 == 0 else 1.0 + 0.01 * j for j in range(M)]
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), M, lens)
        b.synthesize(1234)
        driver.munc_seed_batch(b, pad=PAD, window=WINDOW, passes=1, q=q, exclude=exclude, fit_background=False, fetch=())
        b.synchronize()
        split = dict(block_sums=[], pooled_rows_host=[], prior_track=[], finish=[])
        rows = 0
        for r in range(repeats + 1):            # (the first round warms up: allocations, first-use exports)
            b.stats()
            b.forward_backward(want_sums=False)     # `munc_track_finish` drops the fit: refit outside the clock
            b.synchronize()
            t0 = time.perf_counter()
            sums = b.munc_block_sums(BLOCK)
            t1 = time.perf_counter()
            pooled = MT.pooled_block_rows(sums, dependence_multiplier=2.0)
            t2 = time.perf_counter()
            b.munc_prior_track(trend, floor=FLOOR, cap=CAP)
            b.synchronize()
            t3 = time.perf_counter()
            b.munc_track_finish(NU_L, NU_0, replicate_factors=factors, floor=FLOOR, cap=CAP)
            b.synchronize()
            t4 = time.perf_counter()
            rows = int(pooled["means"].size)
            if r > 0:
                for key, dt in zip(split, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                    split[key].append(dt)
        doc["pooled_rows"] = rows
        doc["blocks"] = int(sum(s["starts"].size for s in sums))
        doc["resident_seconds"] = {k: statistics.median(v) for k, v in split.items()}
        doc["resident_seconds_all"] = split
        doc["resident_device_stages_seconds"] = sum(doc["resident_seconds"][k] for k in ("block_sums", "prior_track", "finish"))
        if host_side:
            import twin_munc_track as T

            b.stats()
            b.forward_backward(want_sums=False)
            smooth, weight = b.download_munc_seed(0, "seed_smooth"), b.download_munc_seed(0, "seed_weight")
            mean = np.ascontiguousarray(b.download(0, "xs")[:, 0])
            n = lens[0]
            drop = dict(block_sums=[], prior_track=[], get_munc_track=[], blacklist_floor=[])
            for _ in range(repeats):
                t0 = time.perf_counter()
                MT.block_sums(smooth, weight, exclude[0], mean.astype(np.float64), BLOCK)
                t1 = time.perf_counter()
                prior = MT.eval_pspline_log_variance_trend(trend, mean, eps=FLOOR, maxVariance=CAP)
                t2 = time.perf_counter()
                out = np.empty((M, n), np.float32)
                iv, vals = np.zeros(n, np.uint32), np.zeros(n, np.float32)
                for j in range(M):
                    out[j], _ = MT.get_munc_track("chr1", iv, vals, 200, eps=FLOOR, varianceFloor=FLOOR, pooledTrend=trend,
                                                  priorMeanTrack=mean, priorVarianceTrack=prior, replicateVarianceFactor=factors[j],
                                                  EB_pooledNu0=NU_0, EB_effectiveNuL=NU_L, localVarianceTrack=smooth[j],
                                                  intervalsArr=iv)
                t3 = time.perf_counter()
                MT.apply_blacklist_munc_floor(out, exclude[0], 1.0e-12)
                t4 = time.perf_counter()
                for key, dt in zip(drop, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                    drop[key].append(dt)
            doc["dropin_seconds"] = {k: statistics.median(v) for k, v in drop.items()}
            doc["dropin_seconds_all"] = drop
            cut = min(twin_blocks * BLOCK, n)
            t0 = time.perf_counter()
            lp = T.block_loop(smooth[:, :cut], weight[:, :cut], exclude[0][:cut], mean[:cut].astype(np.float64), BLOCK)
            dt = time.perf_counter() - t0
            pairs = int(lp["raw"]["starts"].size) * M
            all_pairs = int(sums[0]["starts"].size) * M
            doc["twin_block_loop"] = dict(pairs=pairs, seconds=dt, microseconds_per_pair=1e6 * dt / pairs, chr1_pairs=all_pairs,
                                          chr1_seconds_extrapolated=dt / pairs * all_pairs)
    print(label, json.dumps(doc))
    return doc


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "munc_track_bench.json"))
    ap.add_argument("--chains", type=int, default=22, help="the first N autosomes")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--twin-blocks", type=int, default=1500)
    args = ap.parse_args()

    from consenrich_amd import _lib as L
    from consenrich_amd.sharding import hg38_chain_lengths

    L.require_gpu()
    lens = [int(n) for n in hg38_chain_lengths(200)][:args.chains]
    chr1 = measure(lens[:1], "chr1", args.repeats, True, args.twin_blocks)
    genome = measure(lens, "autosomes", args.repeats, False, args.twin_blocks)
    doc = dict(interval_bp=200, samples=M, block_intervals=BLOCK, trend="degree 3, 60 basis functions (planted)", nu_local=NU_L,
               nu_prior=NU_0, excluded_fraction=0.02, repeats=args.repeats, chr1=chr1, autosomes=genome,
               not_measured=["50 bp", "real data", "the reference's own loop (its natives under its own build, its thread pool)",
                             "kernel counters"],
               note="one process, one MI355X; device-synthesised batch after one seed round; medians of three; the twin's block "
                    "loop is timed on a prefix of chr1 and extrapolated by its pair count")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
