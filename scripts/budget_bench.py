"""Measure the ROCCO budget and gamma from resident scores (csrc/csr_ess.h, csr_host_ess.inl) against the host path they replace.

    python scripts/budget_bench.py          # 1 x MI355X, writes profiles/budget_bench.json (--out)

One process, the 22 hg38 autosomes at 200 bp as one batch with planted score tracks (an AR(1) bulk, phi = 0.9, plus a shifted
tenth), dependence span 64 (lags up to 256), after a warm-up, every timed call ending in a synchronise:
  (a) `DeviceBatch.rocco_budget` (statistic "occupancy", the reference's default) and `DeviceBatch.rocco_gamma` of the batch, three
      runs shown, and the library's event timers per stage (csr_profile_read);
  (b) the path they replace: `download_scores` of every chain, the series with NumPy, scripts/ubench/ess_cpu.c at -O3 on one core,
      and NumPy's median of the positive excess.
The panel behind (a) is not what is measured: its per-z views are made on the host from each chain's null centre and scale
(threshold = centre + z * scale), so that the bench spends its time on the budget.  The results of (a) and (b) are compared bit
for bit.  Also recorded: the lag walk's time with only the longest chain against all chains (the walk is expected to cost what its
longest chain costs)."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

Z_GRID = (1.5, 2.0, 2.5, 3.0)


def planted(n, seed):
    from scipy.signal import lfilter

    rng = np.random.default_rng(seed)
    z = lfilter([1.0], [1.0, -0.9], rng.standard_normal(n)) * 0.4359     # unit variance
    hot = lfilter([1.0], [1.0, -0.98], rng.standard_normal(n)) > 6.4     # about a tenth, in stretches
    z[hot] += 4.0
    return np.ascontiguousarray(z) + 0.0


def cpu_port():
    src = os.path.join(ROOT, "scripts", "ubench", "ess_cpu.c")
    so = os.path.join(tempfile.mkdtemp(prefix="ess_cpu_"), "libess_cpu.so")
    subprocess.check_call(["gcc", "-O3", "-fno-trapping-math", "-fno-math-errno", "-mtune=generic", "-ffp-contract=off", "-shared",
                           "-fPIC", "-o", so, src, "-lm"])
    lib = C.CDLL(so)
    DP = C.POINTER(C.c_double)
    lib.ess_cpu.argtypes = [DP, C.c_long, C.c_long, DP]
    lib.ess_cpu.restype = None

    def ess(series, max_lag):
        x = np.array(series, np.float64)
        out = np.zeros(3)
        lib.ess_cpu(x.ctypes.data_as(DP), x.shape[0], int(max_lag), out.ctypes.data_as(DP))
        return float(out[0]), float(out[1]), int(out[2])

    return ess


def synthetic_panel(center, scale):
    views = []
    for k, z in enumerate(Z_GRID):
        views.append(dict(threshold_z=float(z), threshold=float(center + z * scale), null_center=float(center), null_scale=float(scale),
                          num_bootstrap=8, null_quantile=0.9, observed_tail_occupancy=0.1, null_tail_occupancy=0.02,
                          null_tail_occupancy_calibrated=0.03, null_tail_occupancy_sd=0.01, observed_soft_tail=0.1, null_soft_tail=0.02,
                          null_soft_tail_calibrated=0.03, null_soft_tail_sd=0.01, budget_occupancy_raw=0.07 - 0.01 * k,
                          budget_soft_raw=0.07 - 0.01 * k))
    return views


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "budget_bench.json"))
    ap.add_argument("--chains", type=int, default=22, help="the first N autosomes")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--span", type=int, default=64)
    args = ap.parse_args()

    import twin_budget as T
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams
    from consenrich_amd.sharding import hg38_chain_lengths

    L.require_gpu()
    ess_cpu = cpu_port()
    lens = [int(n) for n in hg38_chain_lengths(200)][:args.chains]
    nc = len(lens)
    tracks = [planted(n, 100 + c) for c, n in enumerate(lens)]
    kw = dict(statistic="occupancy", threshold_z=2.0, threshold_z_grid=Z_GRID, dependence_spans=args.span)
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), 1, lens)
        for c, z in enumerate(tracks):
            b.upload_scores(c, z)
        null = b.rocco_null()
        panel = [synthetic_panel(r["null_center"], r["null_scale"]) for r in null]
        thr = [v[1]["threshold"] for v in panel]
        b.rocco_budget(panel, **kw)             # warm-up: work space, first launches
        b.rocco_gamma(-1.0, dependence_spans=args.span, thresholds=thr)
        b.synchronize()
        b.profile(True)
        wall_b, wall_g = [], []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            budgets = b.rocco_budget(panel, **kw)
            b.synchronize()
            wall_b.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            gammas = b.rocco_gamma(-1.0, dependence_spans=args.span, thresholds=thr)
            b.synchronize()
            wall_g.append(time.perf_counter() - t0)
        kt = b.kernel_times()
        split = {k: dict(launches=v[0] // args.repeats, ms=v[1] / args.repeats) for k, v in sorted(kt.items())
                 if k.startswith(("ess_", "null_"))}
        # the lag walk with the longest chain alone
        b.profile(True)
        longest = int(np.argmax(lens))
        only = [c == longest for c in range(nc)]
        for _ in range(args.repeats):
            b.ess("occupancy", thr, [1.0] * nc, 4 * args.span, chains=only)
        b.synchronize()
        kt1 = b.kernel_times()
        b.profile(False)
        walk_all = split.get("ess_lags", dict(ms=None))["ms"]
        walk_longest = kt1["ess_lags"][1] / args.repeats if "ess_lags" in kt1 else None

        # the path replaced
        t0 = time.perf_counter()
        host_b, host_g, t_down, t_ess, t_med = [], [], 0.0, 0.0, 0.0
        for c in range(nc):
            t1 = time.perf_counter()
            z = b.download_scores(c)
            t2 = time.perf_counter()
            series = (z > thr[c]).astype(np.float64)
            host_b.append(ess_cpu(series, 4 * args.span))
            t3 = time.perf_counter()
            pos = z - thr[c]
            pos = pos[pos > 0.0]
            host_g.append(float(np.median(pos)) if pos.size else 1.0)
            t4 = time.perf_counter()
            t_down, t_ess, t_med = t_down + t2 - t1, t_ess + t3 - t2, t_med + t4 - t3
        t_host = time.perf_counter() - t0
    same = all(T.same_details({"a": budgets[c]["effective_total_count"], "b": budgets[c]["autocorrelation_time"],
                               "c": budgets[c]["ess_lags_used"]}, {"a": host_b[c][0], "b": host_b[c][1], "c": host_b[c][2]}) == []
               and T.same_details({"m": gammas[c][1]["positive_score_median"]}, {"m": host_g[c]}) == [] for c in range(nc))
    dev = min(wall_b) + min(wall_g)
    doc = dict(chains=nc, bins=int(sum(lens)), longest_chain_bins=int(max(lens)), repeats=args.repeats, dependence_span=args.span,
               max_lag=4 * args.span, lags_used=[int(d["ess_lags_used"]) for d in budgets],
               device_rocco_budget_seconds=min(wall_b), device_rocco_budget_seconds_all=wall_b,
               device_rocco_gamma_seconds=min(wall_g), device_rocco_gamma_seconds_all=wall_g,
               host_path_seconds=t_host, host_download_seconds=t_down, host_ess_cpu_seconds=t_ess, host_median_seconds=t_med,
               host_over_device=t_host / dev, results_identical=bool(same), device_ms=split,
               lag_walk_ms_all_chains=walk_all, lag_walk_ms_longest_chain_alone=walk_longest,
               note="one process, one MI355X; host path = download_scores + NumPy series + ess_cpu.c (-O3, one core) + np.median per "
                    "chain; the panel's views are synthetic (threshold = null centre + z * null scale)")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
