#!/usr/bin/env python3
"""Benchmark of the Consenrich estimator hot path on MI355X (driver contract: one JSON line on rank 0).

  python bench.py --gpus N --steps K --warmup W         (N > 1: this process starts its N rank processes itself)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W         (the launcher provides RANK / LOCAL_RANK / WORLD_SIZE / MASTER_PORT)

  python bench.py --config c2|c3|c4|c5                  (one line per BASELINE config; default c4 = the headline)
  python bench.py ... --full                            (also everything beside the headline, see below)
  python bench.py ... --dump-outputs DIR                (after the timed steps: what the last step returned, DIR/<name>.npy)

A plain run sets up, warms up (W steps), times ONE window of exactly K steps and prints the line: `value`, `ms_per_step` and
the workload description.  `--full` adds what takes runs of its own: two more K-step windows (the line then carries the
median window and the spread), per-kernel HIP-event times and the rooflines, the ECM loop, the calibration-fold batch, the
opt-in throughput mode, the CPU baseline and, with N > 1, the final track gather, `per_rank` and `expected`.

Default workload = BASELINE config 4 (BASELINE.json metric "genomic bins/sec (forward+backward pass), hg38 200bp x 32 samples"):
22 synthetic chains with the hg38 autosome bin counts at 200 bp (14 375 018 bins), m = 32 samples, levelTrend model,
SURVEY 8(d) parameters.  c3 = the same chains x 8 samples; c5 = the chains at 50 bp (57 500 042 bins) x 64 samples; c2 = ONE
chain of 1e6 bins x 4 samples, FORWARD FILTER ONLY (statistics + forward(store, NLL) + reference-layout D / xf / Pf / pNoise;
no smoother, no residuals; B_alg = 8 m + 60 bytes per bin; `cpu_baseline` = the port's forward pass alone).
One STEP = one full pass of the hot path over every chain the rank owns, inputs already
resident in HBM:  per-bin sufficient statistics of (data, munc)  ->  forward filter (store, NLL)  ->  RTS smoother
->  lag-one covariances  ->  D, xf, Pf, pNoise, xs, Ps, lagCov in the reference layouts  ->  residuals (n, m).
With N > 1 the chains are LPT-sharded over the ranks (strong scaling: the genome is fixed); there is no data-path
collective -- the one RCCL call is the final track gather, done once after the timed region and reported separately.

`value` is measured in the library's DEFAULT validation mode (x_tol_ulps = 0): the SEQUENTIAL semantics of the library's own
arithmetic -- every speculative block is repaired to the fixed point bit for bit, so results do not depend on blocking.  Against
the REFERENCE that arithmetic differs at ~2^-50 per operation (sufficient statistics hoisted out of the recursion, pyx:271-282;
Newton-refined reciprocals), which flips a float32 rounding of the weakly observed trend a handful of times per genome: on THIS
workload 808 of 2.9e7 filtered-state values differ from the oracle's, all of them trend components off by one ulp of the trend
(1.4e-7 of its RMS), no level, covariance, NIS or residual value differs on any of the 22 chromosomes
(tests/test_gpu_parity.py::test_bench_workload_exact_mode_matches_oracle, profiles/r05_parity_worst_c4_*_exact*.json); after a
6-iteration kappa-ECM on a chr1-sized hard chain every bin stays within 0.10 x the 1e-5 gate (tests/test_hard_data.py).  The
opt-in 2-ulp throughput mode (a single pass within a few float32 ulps of the reference -- half of the filtered values differ in
their last bits --, gated on all 22 chromosomes by test_bench_workload_matches_oracle and on hard data by test_hard_data.py) is
reported beside it as `throughput_mode` (--full).

No PyTorch: a launcher only provides the rank environment; the barrier and the max-over-ranks of the timed region are RCCL
all-reduces on the library's stream (consenrich_amd.sharding.RcclComm -> csr_comm_* in libconsenrich_amd.so, librccl
dlopen'ed there); the 128-byte RCCL id travels through the job's directory on the node (consenrich_amd.launch).  If the RCCL
communicator cannot be created the measurement is still taken (file barrier, `config.comm` = "file") and printed, and the
process exits NON-ZERO: a job whose one collective never came up has failed.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0   # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)
TRAFFIC_FILES = {0: os.path.join("profiles", "r06_pmc_traffic_exact.json"),      # PMC passes of the c4 workload (scripts/pmc_traffic.py)
                 2: os.path.join("profiles", "r06_pmc_traffic.json")}
EXIT_RCCL_FAILED = 3

# BASELINE.json `configs` 2-5 (config 1 is the reference's own CPU-runnable plumbing case: a parity test, not a bench line)
CONFIGS = {
    "c2": {"bin_bp": 200, "samples": 4, "single_chain": 1000000, "forward_only": True,
           "metric": "genomic bins/sec (forward filter only), 1 chromosome of 1e6 x 200bp bins x 4 samples"},
    "c3": {"bin_bp": 200, "samples": 8, "metric": "genomic bins/sec (forward+backward pass), hg38 200bp x 8 samples"},
    "c4": {"bin_bp": 200, "samples": 32, "metric": "genomic bins/sec (forward+backward pass), hg38 200bp x 32 samples"},
    "c5": {"bin_bp": 50, "samples": 64, "metric": "genomic bins/sec (forward+backward pass), hg38 50bp x 64 samples"},
}

# What a rank's step costs as a function of the bins it owns, per validation mode: ms = fixed + per_mbin * (bins / 1e6), fitted to
# the LPT shards of 2 / 4 / 8 ranks emulated on ONE GPU (scripts/shards.sh -> SCALING_MODEL_SOURCE; c4 shape).  The default mode's
# fixed part is the state chain's critical path on the rank's longest chromosome (every rank of <= 8 holds one of chr1..chr8:
# 0.73-1.24 M bins); the throughput mode's is launch / drain latency of its serial kernels.  Used for `expected` at N > 1 only.
SCALING_MODEL = {"default": {"fixed_ms": 1.454, "per_mbin_ms": 0.1650}, "ulp2": {"fixed_ms": 0.124, "per_mbin_ms": 0.1262}}
SCALING_MODEL_SOURCE = "profiles/r06_shards_exact_mode.txt, profiles/r06_shards_throughput_mode.txt (least squares over the five emulated shard sizes)"


PARITY_RECORD = {"c2": "c2_1e6_x4_forward_only_ulp2", "c3": "c3_hg38_200bp_x8_ulp2", "c4": "c4_hg38_200bp_x32_ulp2",
                 "c5": "c5_hg38_50bp_x64_ulp2"}


def throughput_mode_parity(config: str):
    """Which returned arrays the 2-ulp mode holds to north_star's 1e-5 on this workload and which it does not: from the MEASURED
    worst errors the full-size parity test of the config recorded (tests/test_gpu_parity.py -> profiles/rNN_parity_worst_*_ulp2.json,
    the latest round committed; every bin of every checked chain against the oracle)."""
    import glob

    name = PARITY_RECORD.get(config)
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r[0-9][0-9]_parity_worst_{name}.json"))) if name else []
    if not files:
        return None
    with open(files[-1]) as fh:
        w = json.load(fh)
    def worst(*keys):
        vals = [w[k] for k in keys if w.get(k) is not None]
        return max(vals) if vals else None

    held = {"level (xs, xf)": worst("xs_level_rel", "xf_level_rel", "xs"), "uncertainty / Ps": worst("Ps_rel", "unc"),
            "Pf": worst("Pf_rel"), "lag": worst("lag_rel"), "resid": worst("resid_rel"), "NLL": worst("nll_rel"),
            "trend vs the level's scale (the gate)": worst("xs_trend_vs_level", "xf_trend_vs_level")}
    nis = None if w.get("D_frac_outside_1e-5") is None else {"fraction_of_bins": w["D_frac_outside_1e-5"], "worst_relative": w.get("D_rel_max")}
    return {"holds_1e-5": {k: v for k, v in held.items() if v is not None and v <= 1e-5},
            "outside_1e-5": {"NIS": nis if nis is not None else "not recorded for this config (c4: 0.5 % of the bins)",
                             "trend_vs_its_own_rms": worst("xs_trend_vs_trend_rms", "xf_trend_vs_trend_rms")},
            "source": os.path.relpath(files[-1], ROOT), "chains_checked_in_full": w.get("chains_checked_in_full")}


def b_alg(m: int, forward_only: bool = False) -> int:
    """algorithmic bytes per bin, data read once: forward + backward 12 m + 100; forward only 8 m + 60."""
    return 8 * m + 60 if forward_only else 12 * m + 100


def expected_speedup(bins_per_rank, total_bins):
    """`expected` of an N > 1 line: the speed-up over ONE GPU that SCALING_MODEL gives the job's LPT table (slowest rank)."""
    out = {}
    for mode, c in SCALING_MODEL.items():
        t1 = c["fixed_ms"] + c["per_mbin_ms"] * total_bins / 1e6
        tn = max(c["fixed_ms"] + c["per_mbin_ms"] * b / 1e6 for b in bins_per_rank)
        out[mode] = {"speedup_vs_1gpu": t1 / tn, "ms_per_step": tn}
    out["model"] = "ms = fixed + per_mbin * Mbins of the slowest rank; " + json.dumps(SCALING_MODEL)
    out["source"] = SCALING_MODEL_SOURCE
    out["bound"] = ("LPT makespan bound: %.2f x" % (total_bins / max(bins_per_rank)))
    out["note"] = ("default (bit-exact) mode: bounded by the state chain's critical path on each rank's longest chromosome, ~2 x at "
                   "8 GPUs; the opt-in 2-ulp mode (`throughput_mode`) scales to 5.4 x in the emulation (heaviest rank 0.36 ms against "
                   "1.94 ms) -- short of north_star's >= 6 x: a rank's step has ~0.12 ms that does not shrink with its share")
    return out


# algorithmic bytes per bin of each kernel (DESIGN.md "Kernels"): only traffic the reference layouts require
def kernel_alg_bytes(name: str, m: int, d: int) -> float:
    return {
        "stats": 8.0 * m,                       # data + munc read once
        "residuals": 4.0 * m,                   # (n, m) residual write
        "fwd_chain": 16.0 + 16.0 + 16.0 + 8.0,  # lambda/kappa/qscale/blockMap in, Pf + pNoise + xf out (fused chain)
        "fwd_cov_chain": 16.0 + 16.0 + 16.0,    # lambda/kappa/qscale/blockMap in, Pf + pNoise out
        "fwd_state_chain": 8.0,                 # xf out
        "fwd_state": 8.0,                       # bit-exact state chain: speculative pass + repair passes as one unit, xf out
        "fwd_state_seq": 8.0,                   # ... its sequential fallback (CONSENRICH_AMD_SEQ_STATE=1)
        "fwd_dstat": 4.0,                       # D out
        "bwd_chain": 8.0 + 16.0 + 16.0,         # xs + Ps + lagCov out
        "export_natural": 0.0,                  # layout conversion: pure overhead
    }.get(name, 0.0)


def cpu_baseline(m: int, max_seconds: float = 15.0, forward_only: bool = False, n_bins: int = 0):
    """Oracle (C port of the reference loop, 1 thread) on a bounded sample of the same workload: a chr1-sized chain (c2: THE
    1e6-bin chain, forward pass alone).
    (scripts/cpu_port_vs_reference.py, build container only: the port runs within 3 % of the compiled reference.)"""
    import numpy as np

    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import cases
    from consenrich_amd.sharding import hg38_chain_lengths
    from oracle import oracle as orc

    orc.lib()
    n = int(n_bins) if n_bins else hg38_chain_lengths(200)[0]    # chr1-sized chain: 1 244 783 bins
    data, munc = cases.synth(n, m, 21)
    F = np.asarray(cases.F_TREND, np.float32)
    Q0 = np.diag([1e-3, 1e-4]).astype(np.float32)
    bm = (np.arange(n) // 500).astype(np.int32)
    xf, Pf, pn = np.empty((n, 2), np.float32), np.empty((n, 2, 2), np.float32), np.empty((n, 2, 2), np.float32)
    D = np.empty(n, np.float32)
    xs, Ps = np.empty((n, 2), np.float32), np.empty((n, 2, 2), np.float32)
    lag, res = np.empty((n - 1, 2, 2), np.float32), np.empty((n, m), np.float32)

    def one():
        orc.cforwardPass(matrixData=data, matrixPluginMuncInit=munc, matrixF=F, matrixQ0=Q0, intervalToBlockMap=bm,
                         blockCount=int(bm.max()) + 1, stateInit=0.0, stateCovarInit=1000.0, stateForward=xf,
                         stateCovarForward=Pf, pNoiseForward=pn, vectorD=D, returnNLL=True)
        if not forward_only:
            orc.cbackwardPass(matrixData=data, matrixF=F, stateForward=xf, stateCovarForward=Pf, pNoiseForward=pn,
                              stateSmoothed=xs, stateCovarSmoothed=Ps, lagCovSmoothed=lag, postFitResiduals=res)

    one()  # warm-up (first-touch page faults)
    best, spent, reps = float("inf"), 0.0, 0
    while reps < 400 and spent < max_seconds:
        t = time.perf_counter()
        one()
        dt = time.perf_counter() - t
        best = min(best, dt)
        spent += dt
        reps += 1
    return {
        "value": n / best, "unit": "genomic bins/s", "cores": 1, "host_cores": os.cpu_count(), "kind": "port",
        "sample": f"oracle C port ({'forward store+NLL only' if forward_only else 'forward store+NLL, backward+residuals'}), "
                  f"1 thread, {'the' if n_bins else 'chr1-sized'} chain "
                  f"({n} bins x {m} samples), best of {reps} passes after warm-up ({spent:.1f} s of CPU work)",
    }


DUMP_BUDGET_BYTES = 60 * 2**20     # below the 64 MB a dump may hold in all
DUMP_MAX_ROWS = 1 << 17            # sampled bins (and bin-to-bin transitions) per job
DUMP_SEED = 20240607


def dump_outputs(batch, lens, forward_only: bool, sums, out_dir: str, prefix: str = "", share: int = 1):
    """Write what the last timed step returned (`sums` = its per-chain (sumD, sumNLL)) and the arrays it exported, as
    out_dir/<prefix><name>.npy.  Per-bin arrays (D, xf, Pf, and unless forward-only xs, Ps, resid) hold the rows of a fixed,
    seeded sample of the batch's bins, in bin order over the chains as configured; pNoise and lagCov (n - 1 rows per chain)
    those of a sample of the transitions.  Same arguments -> same sample."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    d, m = batch.d, batch.m
    per_bin = ["D", "xf", "Pf"] + ([] if forward_only else ["xs", "Ps", "resid"])
    per_step = ["pnoise"] + ([] if forward_only else ["lag"])
    row_shape = {"D": (), "xf": (d,), "Pf": (d, d), "xs": (d,), "Ps": (d, d), "resid": (m,), "pnoise": (d, d), "lag": (d, d)}
    row_bytes = 4 * sum(int(np.prod(row_shape[k])) for k in per_bin + per_step)
    rows = max(1, min(DUMP_MAX_ROWS, DUMP_BUDGET_BYTES // (row_bytes * max(share, 1))))
    rng = np.random.default_rng(DUMP_SEED)

    def sample(counts):
        total = int(sum(counts))
        idx = np.sort(rng.choice(total, size=min(rows, total), replace=False)) if total else np.zeros(0, np.int64)
        starts = np.concatenate([[0], np.cumsum(counts)])
        chain = np.searchsorted(starts, idx, side="right") - 1
        return chain, idx - starts[chain]

    out = {}
    for names, counts in ((per_bin, list(lens)), (per_step, [max(n - 1, 0) for n in lens])):
        chain, local = sample(counts)
        for name in names:
            parts = [np.zeros((0, *row_shape[name]), np.float32)]
            for c in np.unique(chain):
                parts.append(batch.download(int(c), name)[local[chain == c]])
            out[name] = np.concatenate(parts)
    out["sumD"], out["sumNLL"] = (np.asarray(s, np.float64) for s in sums)
    for name, arr in out.items():
        np.save(os.path.join(out_dir, f"{prefix}{name}.npy"), arr)
    return sorted(out)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", choices=sorted(CONFIGS), default="c4",
                    help="BASELINE config: c2 = 1 chain of 1e6 bins x 4, forward filter only; c3 = hg38 @200bp x 8; "
                         "c4 = hg38 @200bp x 32 (default, the headline); c5 = hg38 @50bp x 64")
    ap.add_argument("--samples", type=int, default=None, help="override the config's sample count")
    ap.add_argument("--bin-bp", type=int, default=None, help="override the config's bin size")
    ap.add_argument("--q0", default="1e-3,1e-4", help="diagonal of the base process noise Q0 (long-memory regime: 1e-5,1e-6)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: three timed windows, per-kernel times and rooflines, the extras, the CPU "
                         "baseline, and with N > 1 the track gather, per_rank and expected")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step returned to DIR/<name>.npy (a fixed, seeded "
                         "sample of the per-bin arrays; at most 64 MB in all)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-gather", action="store_true", help="with --full: skip the final track gather")
    ap.add_argument("--no-extras", action="store_true",
                    help="with --full: skip the throughput-mode, ECM and calibration-fold measurements")
    ap.add_argument("--same-device", action="store_true", help="rehearsal: every rank uses GPU 0 (no RCCL: file barrier)")
    ap.add_argument("--fake-ranks", action="store_true",
                    help="CPU rehearsal of the launcher and control plane: no GPU, no measurement; rank 0 prints a stub line")
    args = ap.parse_args(argv)
    if args.dump_outputs and args.steps < 1:
        ap.error("--dump-outputs writes what the last timed step returned: needs --steps >= 1")
    cfg = CONFIGS[args.config]
    if args.samples is None:
        args.samples = cfg["samples"]
    if args.bin_bp is None:
        args.bin_bp = cfg["bin_bp"]
    args.forward_only = bool(cfg.get("forward_only"))
    args.single_chain = int(cfg.get("single_chain", 0))
    args.metric = cfg["metric"] if (args.samples == cfg["samples"] and args.bin_bp == cfg["bin_bp"]) else \
        f"genomic bins/sec (forward+backward pass), hg38 {args.bin_bp}bp x {args.samples} samples"
    return args


def fake_rank(args) -> int:
    """What `--fake-ranks` runs in every rank: the job's control plane without a GPU (tests/test_launch.py)."""
    from consenrich_amd.launch import JobFiles

    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    files = JobFiles(rank, world)
    seen = files.allreduce_sum(1.0, timeout_s=60.0)
    slowest = files.allreduce_max(float(rank), timeout_s=60.0)
    fail = os.environ.get("CONSENRICH_AMD_FAKE_FAIL_RANK")
    files.close(remove=False)
    if rank == 0:
        print(json.dumps({"fake": True, "n_gpus": world, "n_ranks_seen": int(round(seen)), "max_rank": int(slowest)}))
    return 5 if fail is not None and int(fail) == rank else 0


def main() -> int:
    args = parse_args()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # started plainly: become the launcher of N rank processes (nothing in this process has touched the GPU)
        from consenrich_amd.launch import spawn_ranks

        return spawn_ranks([sys.executable, os.path.abspath(__file__), *sys.argv[1:]], args.gpus)
    if args.fake_ranks:
        return fake_rank(args)

    import numpy as np

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = 0 if args.same_device else int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE is {world}", file=sys.stderr)
        return 2

    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams
    from consenrich_amd.launch import JobFiles
    from consenrich_amd.sharding import RcclComm, hg38_chain_lengths, lpt_assign

    L.require_gpu()          # no GPU, no number: there is no CPU fallback to time
    m = args.samples
    q00, q11 = (float(v) for v in args.q0.split(","))
    lengths = [args.single_chain] if args.single_chain else hg38_chain_lengths(args.bin_bp)
    if world > len(lengths):
        print(f"bench.py: --config {args.config} has {len(lengths)} chain(s): nothing to shard over {world} GPUs", file=sys.stderr)
        return 2
    total_bins = int(sum(lengths))
    mine = lpt_assign(lengths, world)[rank]
    my_lens = [lengths[i] for i in mine]
    my_bins = int(sum(my_lens))

    model = ModelParams(state_dim=2, Q0=((q00, 0.0), (0.0, q11)))
    batch = DeviceBatch(local_rank)                          # the library's default validation mode (bit-exact)
    comm, comm_kind, comm_note, files, rccl_failed, rccl_hung = None, "none", None, None, False, False
    n_ranks_seen = 1
    if world > 1:
        files = JobFiles(rank, world)
        if args.same_device:
            comm, comm_kind = files, "file"
            comm_note = "same-device rehearsal: RCCL refuses two ranks on one GPU"
        else:
            # communicator creation is a collective: under a watchdog, so that a bootstrap that never completes still leaves a
            # measurement (taken over the file barrier) and a diagnosis -- and a non-zero exit status
            import threading

            box = {}

            def make():
                try:
                    box["comm"] = RcclComm(batch, world, rank, files=files)
                except Exception as exc:        # noqa: BLE001
                    box["err"] = repr(exc)

            th = threading.Thread(target=make, daemon=True)
            th.start()
            th.join(timeout=float(os.environ.get("CONSENRICH_AMD_RCCL_TIMEOUT", "240")))
            mine_ok = "comm" in box
            if files.allreduce_max(0.0 if mine_ok else 1.0) == 0.0:
                comm, comm_kind = box["comm"], "rccl"
                n_ranks_seen = comm.ranks_seen()
            else:
                comm, comm_kind, rccl_failed = files, "file", True
                rccl_hung = th.is_alive()
                comm_note = (f"rank {rank}: RCCL communicator not created ({box.get('err', 'timeout inside ncclCommInitRank')})"
                             if not mine_ok else "RCCL communicator not created on another rank")
        if comm_kind == "file":
            n_ranks_seen = int(round(files.allreduce_sum(1.0)))
    batch.configure(model, m, my_lens)
    batch.synthesize(seed=1234 + rank)
    flags = L.RETURN_NLL
    what = L.EXPORT_FORWARD if args.forward_only else (L.EXPORT_FORWARD | L.EXPORT_SMOOTH | L.EXPORT_RESID)
    bytes_per_bin = b_alg(m, args.forward_only)

    def one_step(b):
        # c2: the forward filter alone (statistics + forward(store, NLL) + its tracks in the reference layouts)
        return b.step_forward(flags, what) if args.forward_only else b.step(flags, what)

    def fence(b=batch):
        # device-wide synchronize of this rank, then the barrier over all ranks (an RCCL all-reduce on the library's
        # stream + stream synchronisation), then nothing is in flight anywhere
        b.synchronize()
        if comm is not None:
            comm.barrier()

    def max_over_ranks(v: float) -> float:
        return comm.allreduce_max(v) if comm is not None else v

    last = {}

    def timed(b, fn, warmup, steps):
        for _ in range(warmup):
            fn()
        fence(b)
        t0 = time.perf_counter()
        for _ in range(steps):
            last["ret"] = fn()
        fence(b)
        return max_over_ranks(time.perf_counter() - t0)

    def profile_kernels(b, steps):
        """per-kernel durations: HIP events on the library's stream, separate (untimed) pass of the same steps"""
        b.profile(True)
        for _ in range(steps):
            one_step(b)
        times = b.kernel_times()
        b.profile(False)
        return {k: {"launches": v[0], "avg_ms": v[1] / max(v[0], 1), "ms_per_step": v[1] / max(steps, 1)} for k, v in times.items()}

    def roofline_of(per_kernel, xtol):
        # dominant kernel = the longest one ON THE CRITICAL PATH: the NIS/NLL epilogue runs on the side stream underneath the
        # smoother / residual kernels (its event-measured duration is stretched by that overlap), so it never is.  The
        # bit-exact state chain is ONE unit of work -- one launch (k_sb_async), or a speculative pass + repair passes
        # (`fwd_state_chain` + `fwd_state_fix`) when the barrier-free form is switched off: priced as such (bytes of the unit /
        # time of the unit per step).
        crit = {k: dict(v) for k, v in per_kernel.items() if k != "fwd_dstat"}
        if xtol == 0 and "fwd_state_chain" in crit:
            a = crit.pop("fwd_state_chain")
            f = crit.pop("fwd_state_fix", None)     # CONSENRICH_AMD_SB_ASYNC=0: repair passes as launches of their own
            if f is None:
                crit["fwd_state"] = a               # the barrier-free form: ONE launch per step (k_sb_async)
            else:
                crit["fwd_state"] = {"launches": a["launches"] + f["launches"], "ms_per_step": a["ms_per_step"] + f["ms_per_step"],
                                     "avg_ms": a["ms_per_step"] + f["ms_per_step"]}       # one unit per step
        if not crit:
            return None
        dom = max(crit, key=lambda k: crit[k]["ms_per_step"])
        alg_bytes = kernel_alg_bytes(dom, m, 2) * my_bins
        avg_s = crit[dom]["avg_ms"] * 1e-3
        achieved = alg_bytes / avg_s / 1e9 if avg_s > 0 else 0.0
        traffic, traffic_source = None, None
        pmc_path = os.path.join(ROOT, TRAFFIC_FILES.get(xtol, ""))
        # a committed PMC pass describes the default workload at N = 1 only
        if os.path.isfile(pmc_path) and world == 1 and args.config == "c4" and m == 32 and args.bin_bp == 200 and args.q0 == "1e-3,1e-4":
            try:
                with open(pmc_path) as fh:
                    traffic = json.load(fh).get(dom, {}).get("hbm_bytes_per_launch")
                traffic_source = f"{TRAFFIC_FILES[xtol]} (rocprofv3 --pmc FETCH_SIZE x2 / WRITE_SIZE, separate passes of this " \
                                 "command; not measured in this run)"
            except Exception:       # noqa: BLE001
                traffic = None
        out = {"bound": "hbm", "kernel": dom, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
               "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_source,
               "alg_bytes_per_bin": kernel_alg_bytes(dom, m, 2), "bins_per_launch": my_bins,
               "avg_launch_ms": crit[dom]["avg_ms"], "launches_per_step": crit[dom]["launches"] / max(args.steps, 1)}
        if dom == "fwd_state":
            out["limit"] = ("instruction issue of ONE wavefront per SIMD, not bandwidth: the exact float32-rounded state recursion is "
                            "sequential per chain; a wavefront issues one instruction per ~5 cycles whatever its type "
                            "(scripts/ubench/issue_cost.hip), the walk costs 12 instructions per bin (~30 ns), a re-run in delta "
                            "form ~5 per bin (~14 ns); the launch lasts as long as the true trajectory needs to meet a speculative "
                            "one on the slowest chain (DESIGN.md section 3)")
        return out

    # ---- the headline: the library's default mode --------------------------------------------------------------------
    # a timed window of exactly K steps (bracketed by barrier + synchronize, max over ranks).  --full times three such windows
    # and the line carries the MEDIAN one (a latency-bound step's time depends on which chain is the unlucky one: box-to-box
    # and window-to-window spread is several per cent) and the spread beside it
    n_windows = 3 if args.full else 1
    windows = sorted(timed(batch, lambda: one_step(batch), args.warmup if w == 0 else 0, args.steps) for w in range(n_windows))
    elapsed = windows[len(windows) // 2]
    ms_per_step = 1000.0 * elapsed / max(args.steps, 1)
    value = total_bins * args.steps / elapsed
    dumped = None
    if args.dump_outputs:
        # what the last timed step returned, before anything else runs on this batch
        dumped = dump_outputs(batch, my_lens, args.forward_only, last["ret"], args.dump_outputs,
                              prefix="" if world == 1 else f"rank{rank}_", share=world)
    per_kernel = profile_kernels(batch, args.steps) if args.full else {}
    rs = batch.run_stats()
    roofline = roofline_of(per_kernel, rs["x_tol_ulps"])
    # the dominant bandwidth-bound kernel beside it (what an HBM roofline is meaningful for)
    # (the one with the most algorithmic bytes: the sufficient statistics.  The residual kernel shares the chip with the NIS/NLL
    # epilogue of the side stream, which stretches its event-measured duration)
    stream = {k: v for k, v in per_kernel.items() if k in ("stats", "residuals")}
    roofline_streaming = None
    if stream:
        sk = max(stream, key=lambda k: kernel_alg_bytes(k, m, 2))
        ach = kernel_alg_bytes(sk, m, 2) * my_bins / (stream[sk]["avg_ms"] * 1e-3) / 1e9
        roofline_streaming = {"bound": "hbm", "kernel": sk, "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                              "frac": ach / HBM_PEAK_GBS, "alg_bytes_per_bin": kernel_alg_bytes(sk, m, 2),
                              "avg_launch_ms": stream[sk]["avg_ms"]}

    extras = {}
    ecm_iters, inner = 3, 5

    def ecm_once(b=batch):
        b.ecm(max_iters=ecm_iters, inner_iters=inner, rtol=0.0, use_lambda=False, use_kappa=True)

    # what fits: c2 is a forward-only line (no ECM, no folds); three more copies of c5 (59 GB each) beside the two resident
    # batches would not leave headroom in 288 GB
    do_ecm = args.full and not args.no_extras and not args.forward_only
    do_folds = do_ecm and my_bins * (16.0 * m + 400.0) * 4.0 < 200e9
    if do_ecm:
        # (1) the ECM loop -- what real runs execute: 5 x [forward, smoother + kappa E-step] + 1 NLL forward
        batch.stats()
        e = timed(batch, ecm_once, 1, 2) / 2.0
        extras["ecm"] = {"x_tol_ulps": rs["x_tol_ulps"], "ms_per_iter": 1000.0 * e / ecm_iters, "iters": ecm_iters,
                         "inner_sweeps": inner, "bin_sweeps_per_s": total_bins * ecm_iters * inner / e,
                         "note": "per ECM iteration over all chains: 5 x (forward + smoother + kappa E-step) + 1 NLL "
                                 "forward; bin_sweeps = forward+backward+E-step sweeps; default (bit-exact) mode"}
    if do_folds:
        # (2) the same step with the delete-block calibration folds of every chromosome as extra chains of the batch
        # (uncertainty.py:1370-1419: folds = 2 independent refits per chromosome, constants.py:437; DeviceBatch.make_fold):
        # independent chains fill the GPU the latency-bound exact state chain leaves idle -- also the weak-scaling line of an
        # N > 1 job (every rank triples its own chains)
        folds = 2
        fb = DeviceBatch(local_rank)
        fb.configure(model, m, [n for n in my_lens for _ in range(folds + 1)])
        fb.synthesize(seed=4321 + rank)
        fsteps = max(1, min(args.steps, 3))
        ef = timed(fb, lambda: fb.step(flags, what), 1, fsteps)
        extras["with_calibration_folds"] = {"x_tol_ulps": rs["x_tol_ulps"], "folds": folds, "ms_per_step": 1000.0 * ef / fsteps,
                                            "value": total_bins * (folds + 1) * fsteps / ef, "unit": "genomic bins/s",
                                            "note": "every chromosome three times in the batch (fit + 2 fold refits, "
                                                    "synthetic data of the same shape); bins of all refits counted"}
        fb.stats()
        efe = timed(fb, lambda: ecm_once(fb), 1, 1)
        extras["with_calibration_folds"]["ecm_ms_per_iter"] = 1000.0 * efe / ecm_iters
        extras["with_calibration_folds"]["ecm_bin_sweeps_per_s"] = total_bins * (folds + 1) * ecm_iters * inner / efe
        fb.close()
    if args.full and not args.no_extras:
        # (3) the opt-in throughput mode (2-ulp carry acceptance): same step, same outputs within a few float32 ulps
        tb = DeviceBatch(local_rank, x_tol_ulps=2)
        tb.configure(model, m, my_lens)
        tb.synthesize(seed=1234 + rank)
        et = timed(tb, lambda: one_step(tb), args.warmup, args.steps)
        tk = profile_kernels(tb, args.steps)
        trs = tb.run_stats()
        tvalue = total_bins * args.steps / et
        ete = None
        if do_ecm:
            tb.stats()
            ete = timed(tb, lambda: ecm_once(tb), 1, 2) / 2.0
        extras["throughput_mode"] = {
            "x_tol_ulps": 2, "ms_per_step": 1000.0 * et / max(args.steps, 1), "value": tvalue, "unit": "genomic bins/s",
            "roofline": roofline_of(tk, 2),
            "path_roofline": {"alg_bytes_per_bin": bytes_per_bin, "achieved": tvalue * bytes_per_bin / 1e9,
                              "peak": HBM_PEAK_GBS * world, "unit": "GB/s",
                              "frac": tvalue * bytes_per_bin / 1e9 / (HBM_PEAK_GBS * world)},
            "ecm_ms_per_iter": None if ete is None else 1000.0 * ete / ecm_iters,
            "block_len": trs["block_len"], "warm_bins": [trs["warm_p"], trs["warm_x"], trs["warm_b"]],
            "reruns": [trs["reruns_p"], trs["reruns_x"], trs["reruns_b"]], "pipeline_redos": trs["pipeline_redos"],
            "kernels_rank0": tk,
            "parity": throughput_mode_parity(args.config),
            "contract": "opt-in (DeviceBatch(x_tol_ulps=2)): a speculative carry is accepted within 2 float32 ulps; a single "
                        "pass stays within a few ulps of the reference on every bin, also on hard data "
                        "(tests/test_hard_data.py); iterated through the ECM loop on ill-conditioned data it inherits the "
                        "reference's own sensitivity to ulp-level perturbations, which is why it is not the default"}
        tb.close()

    # what a measured scaling curve has to be read against: every rank's state-chain time and longest chromosome
    def per_rank(v: float):
        if comm is None:
            return [v]
        return [comm.allreduce_sum(v if r == rank else 0.0) for r in range(world)]

    ranks_info = None
    if args.full:
        state_ms = (roofline or {}).get("avg_launch_ms", 0.0) if (roofline or {}).get("kernel") == "fwd_state" else \
            per_kernel.get("fwd_state_chain", {}).get("ms_per_step", 0.0)
        ranks_info = {"fwd_state_ms": per_rank(float(state_ms)), "longest_chain_bins": [int(v) for v in per_rank(float(max(my_lens)))],
                      "bins": [int(v) for v in per_rank(float(my_bins))]}

    gather_ms, gather_note = None, comm_note
    if args.full and comm_kind == "rccl" and not args.no_gather:
        # final track gather (state + its variance): once per job, packed on the device from the exported arrays and
        # all-gathered over RCCL / xGMI; not part of `value`.  A failure here must not cost the measurement its JSON line.
        try:
            batch.step(flags, L.EXPORT_FORWARD | L.EXPORT_SMOOTH | L.EXPORT_RESID)
            fence()
            tg = time.perf_counter()
            gathered = comm.gather_batch_tracks(lengths, to_host=True)
            fence()
            gather_ms = 1000.0 * max_over_ranks(time.perf_counter() - tg)
            if rank == 0 and not all(g is not None and g.shape == (lengths[i], 2) and np.all(np.isfinite(g))
                                     for i, g in enumerate(gathered)):
                gather_note = "gathered tracks have unexpected shapes / values"
                rccl_failed = True
        except Exception as exc:        # noqa: BLE001
            gather_note = f"gather failed: {exc!r}"
            rccl_failed = True

    if rank == 0:
        out = {
            "metric": args.metric,
            "value": value, "unit": "genomic bins/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "ms_per_step_min": 1000.0 * windows[0] / max(args.steps, 1),
            "ms_per_step_median": ms_per_step, "ms_per_step_max": 1000.0 * windows[-1] / max(args.steps, 1),
            "timed_windows": n_windows,
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": "f64 arithmetic on f32 storage", "data": "synthetic",
            "config": {
                "baseline_config": args.config,
                "workload": (f"ONE chain of {total_bins} bins @{args.bin_bp}bp x {m} samples; FORWARD FILTER ONLY: stats + "
                             "forward(store,NLL) + D / xf / Pf / pNoise in the reference layouts (no smoother, no residuals), "
                             "levelTrend, constant process noise" if args.forward_only else
                             f"hg38 autosomes, 22 chains / {total_bins} bins @{args.bin_bp}bp x {m} samples; "
                             "stats + forward(store,NLL) + RTS backward + lagCov + reference-layout tracks + residuals, "
                             "levelTrend, constant process noise (no per-bin lambda / kappa / qScale, one Q0 for every chain: "
                             "the case of a plain forward + backward call; the ECM loop's sweeps carry kappa per bin and are "
                             "reported under `ecm` with --full)"),
                "mfma": "not eligible: the observation update is a length-m weighted reduction per bin (pyx:443-456), no dense "
                        "contraction at any m; the bound is HBM",
                "chains_per_rank": "LPT over contigs", "block_len": rs["block_len"], "q0_diag": [q00, q11],
                "warm_bins": [rs["warm_p"], rs["warm_x"], rs["warm_b"]], "x_tol_ulps": rs["x_tol_ulps"],
                "validation": "bit-exact sequential semantics (library default)" if rs["x_tol_ulps"] == 0
                              else f"{rs['x_tol_ulps']}-ulp carry acceptance",
                "comm": comm_kind, "n_ranks_seen": n_ranks_seen,
            },
            "build": L.build_id(),
            "path_roofline": {"alg_bytes_per_bin": bytes_per_bin, "achieved": value * bytes_per_bin / 1e9,
                              "peak": HBM_PEAK_GBS * world, "unit": "GB/s",
                              "frac": value * bytes_per_bin / 1e9 / (HBM_PEAK_GBS * world)},
            "speculation": {"blocks": rs["blocks"], "reruns_cov": rs["reruns_p"], "reruns_state": rs["reruns_x"],
                            "reruns_bwd": rs["reruns_b"], "fix_launches": rs["fix_launches"],
                            "pipeline_redos": rs["pipeline_redos"],
                            # bit-exact steps: groups of chains whose tail was launched on its own (step_pipelined), and single
                            # launches of the state chain that gave up on a bounded wait (the pass form ran instead)
                            "tail_groups": rs.get("tail_groups", 0), "state_chain_bailouts": rs.get("sb_bailouts", 0)},
            "full": bool(args.full),
        }
        if dumped is not None:
            out["dumped_outputs"] = dumped
        if args.full:
            out.update({"roofline": roofline, "roofline_streaming": roofline_streaming, "kernels_rank0": per_kernel,
                        "gather_ms": gather_ms, "per_rank": ranks_info})
        out.update(extras)
        if args.full and world > 1 and args.config == "c4":
            out["expected"] = expected_speedup(ranks_info["bins"], total_bins)
            # measured against the model: > 1 = faster than the emulated shards said
            out["speedup_vs_expected"] = out["expected"]["default"]["ms_per_step"] / ms_per_step
            if "throughput_mode" in out:
                out["throughput_mode"]["speedup_vs_expected"] = out["expected"]["ulp2"]["ms_per_step"] / out["throughput_mode"]["ms_per_step"]
        if gather_note:
            out["gather_note"] = gather_note
        if args.full and not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(m, forward_only=args.forward_only, n_bins=args.single_chain)
        print(json.dumps(out))
        sys.stdout.flush()
    status = EXIT_RCCL_FAILED if rccl_failed else 0
    if rccl_hung:
        # a thread of this process is still inside ncclCommInitRank: a normal interpreter exit would wait for it.  The line is
        # out; leave with the failure status.
        if files is not None:
            try:
                files.close()
            except Exception:       # noqa: BLE001
                pass
        os._exit(status)
    if comm is not None:
        comm.barrier()
    batch.close()                   # closes the RCCL communicator attached to it, then the context
    if files is not None:
        files.close()
    return status


if __name__ == "__main__":
    raise SystemExit(main())
