"""ROCCO peak selection of a whole genome on the device vs the same sequential algorithm on one CPU core.

Workload: the 22 chain lengths of BASELINE config 4 (hg38 autosomes at 200 bp, 14.4 M bins), scores = the smoothed level of the
synthesized fit, budget 0.03, gamma 0.5, maxIter 60.  GPU: DeviceBatch.rocco_scores + rocco (all chains and, per round, the
2^D - 1 penalties the next D bisection steps can visit, side by side), for D in --depths.  CPU: scripts/ubench/rocco_cpu.c,
this project's plain-C restatement built with the reference's flags, chain after chain on ONE core (the machine's core count
is printed beside it).  Where the compiled reference natives exist (oracle/_ref, build image only) the C port is also timed
against them on one chain, which says how honest the CPU column is.  Prints one JSON line; --out writes it to a file too.

    python scripts/rocco_bench.py [--depths 6,1,8] [--samples 4] [--scale 1] [--cpu-chains 22] [--out profiles/rocco_bench.json]
"""
import argparse, ctypes as C, json, os, subprocess, sys, tempfile, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R)
import numpy as np


def cpu_port():
    src = os.path.join(R, "scripts", "ubench", "rocco_cpu.c")
    so = os.path.join(tempfile.mkdtemp(prefix="rocco_cpu_"), "librocco_cpu.so")
    subprocess.check_call(["gcc", "-O3", "-fno-trapping-math", "-fno-math-errno", "-mtune=generic", "-ffp-contract=off", "-shared",
                           "-fPIC", "-o", so, src, "-lm"])
    lib = C.CDLL(so)
    lib.rocco_chrom.restype = C.c_int64
    lib.rocco_chrom.argtypes = [C.POINTER(C.c_double), C.c_int64, C.c_double, C.c_double, C.c_int, C.POINTER(C.c_double),
                                C.POINTER(C.c_uint8)]

    def run(s, budget, gamma, max_iter):
        out, sol = np.empty(4), np.empty(s.size, np.uint8)
        passes = lib.rocco_chrom(s.ctypes.data_as(C.POINTER(C.c_double)), s.size, budget, gamma, max_iter,
                                 out.ctypes.data_as(C.POINTER(C.c_double)), sol.ctypes.data_as(C.POINTER(C.c_uint8)))
        return (sol, float(out[2]), float(out[1]), int(out[3]), float(out[0])), int(passes)
    return run


def same(a, b):
    return (np.array_equal(a[0], b[0]) and a[3] == b[3] and
            np.array_equal(np.array([a[1], a[2], a[4]]).view(np.uint64), np.array([b[1], b[2], b[4]]).view(np.uint64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depths", default="6,1,8")
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--scale", type=int, default=1, help="divide every chain length by this (quick runs)")
    ap.add_argument("--cpu-chains", type=int, default=22, help="how many chains the CPU column times (the rest is extrapolated by bins)")
    ap.add_argument("--no-gpu", action="store_true", help="only the CPU port against the compiled reference")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    budget, gamma, max_iter = 0.03, 0.5, 60
    cpu = cpu_port()
    row = {"row": "ROCCO peak selection, hg38 @200bp", "budget": budget, "gamma": gamma, "max_iter": max_iter,
           "host_cores": os.cpu_count(), "cpu_cores_used": 1}
    sys.path.insert(0, os.path.join(R, "tests"))
    from oracle import ref_loader
    ref = ref_loader.load()
    if ref is not None:         # how honest is the CPU column: the C port against the compiled reference, one chain
        s = np.cumsum(np.random.default_rng(0).normal(0, 0.03, 400000 // a.scale))
        t = time.perf_counter(); want = ref.csolveChromROCCOExact(s, budget=budget, gamma=gamma, maxIter=max_iter); t_ref = time.perf_counter() - t
        t = time.perf_counter(); got, passes = cpu(s, budget, gamma, max_iter); t_c = time.perf_counter() - t
        row["c_port_vs_reference"] = {"bins": int(s.size), "reference_ms": round(t_ref * 1e3, 1), "c_port_ms": round(t_c * 1e3, 1),
                                      "reference_over_c_port": round(t_ref / t_c, 3), "bit_identical": same(got, want),
                                      "c_port_ns_per_step": round(t_c * 1e9 / (passes * s.size), 2)}
    if not a.no_gpu:
        from consenrich_amd import _lib as L
        from consenrich_amd.batch import DeviceBatch, ModelParams
        from consenrich_amd.sharding import hg38_chain_lengths
        lens = [max(1, n // a.scale) for n in hg38_chain_lengths(200)]
        row.update(chains=len(lens), bins=int(sum(lens)), longest_chain=int(max(lens)), samples=a.samples)
        b = DeviceBatch(0); b.configure(ModelParams(state_dim=2), a.samples, lens); b.synthesize(1)
        b.step(L.RETURN_NLL, L.EXPORT_SMOOTH); b.synchronize()
        t = time.perf_counter(); b.rocco_scores("state"); row["gpu_scores_ms"] = round((time.perf_counter() - t) * 1e3, 2)
        first, row["gpu"] = None, []
        for D in [int(v) for v in a.depths.split(",")]:
            b.set_rocco_depth(D)
            b.rocco(budget=budget, gamma=gamma, max_iter=max_iter)       # warm-up (allocations)
            s0 = b.rocco_stats(); b.profile(True)
            t = time.perf_counter(); res = b.rocco(budget=budget, gamma=gamma, max_iter=max_iter); wall = time.perf_counter() - t
            kt = b.kernel_times(); b.profile(False); s1 = b.rocco_stats()
            rounds = s1["rounds"] - s0["rounds"]
            row["gpu"].append({"D": s1["depth"], "total_ms": round(wall * 1e3, 2), "rounds": rounds, "ms_per_round": round(wall * 1e3 / rounds, 2),
                               "launches": s1["launches"] - s0["launches"], "h2d_bytes": s1["h2d_bytes"] - s0["h2d_bytes"],
                               "d2h_bytes": s1["d2h_bytes"] - s0["d2h_bytes"], "lane_steps": s1["lane_steps"] - s0["lane_steps"],
                               # count-only walks alone: their kernel time over (their launches x the longest chain's steps)
                               "count_walk_ns_per_step": round(kt["rocco_count"][1] * 1e6 / (kt["rocco_count"][0] * max(lens)), 2),
                               "kernel_ms": {k: round(v[1], 2) for k, v in kt.items() if k.startswith("rocco_")}})
            rec = [(b.rocco_solution(c), r["objective"], r["penalized_objective"], r["selected_count"], r["selection_penalty"]) for c, r in enumerate(res)]
            if first is None:
                first = rec
            row["gpu"][-1]["same_as_first_depth"] = all(same(x, y) for x, y in zip(rec, first))
        t = time.perf_counter(); runs = [b.rocco_runs(c, 0) for c in range(len(lens))]; row["gpu_runs_ms"] = round((time.perf_counter() - t) * 1e3, 2)
        row["peaks"] = int(sum(len(r[0]) for r in runs)); row["mask_bytes_not_fetched"] = int(sum(lens)); row["run_bytes_fetched"] = 16 * row["peaks"]
        # CPU column: the same scores, chain after chain, one core
        order = sorted(range(len(lens)), key=lambda c: lens[c])[: a.cpu_chains]
        t_cpu, bins_cpu, ok, passes = 0.0, 0, True, 0
        for c in order:
            s = b.download_scores(c)
            t = time.perf_counter(); got, p_ = cpu(s, budget, gamma, max_iter); t_cpu += time.perf_counter() - t
            bins_cpu += lens[c]; passes += p_ * lens[c]; ok = ok and same(got, first[c])
        row["cpu"] = {"chains_timed": len(order), "bins_timed": bins_cpu, "ms": round(t_cpu * 1e3, 1), "ns_per_step": round(t_cpu * 1e9 / passes, 2),
                      "ms_all_chains_by_bins": round(t_cpu * 1e3 * sum(lens) / bins_cpu, 1), "bit_identical_to_gpu": ok}
        best = min(g["total_ms"] for g in row["gpu"])
        row["cpu_one_core_over_gpu_batch"] = round(row["cpu"]["ms_all_chains_by_bins"] / best, 2)
        # a single chain alone (the longest): is one chain faster than one CPU core?
        b.set_rocco_depth(0)
        cm = [c == int(np.argmax(lens)) for c in range(len(lens))]
        t = time.perf_counter(); b.rocco(budget=budget, gamma=gamma, max_iter=max_iter, chains=cm); t1 = time.perf_counter() - t
        s = b.download_scores(int(np.argmax(lens)))
        t = time.perf_counter(); cpu(s, budget, gamma, max_iter); t1c = time.perf_counter() - t
        row["single_longest_chain"] = {"bins": int(max(lens)), "gpu_ms": round(t1 * 1e3, 1), "cpu_one_core_ms": round(t1c * 1e3, 1)}
        b.close()
    line = json.dumps(row)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
