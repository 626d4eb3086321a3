"""The stationary-null DWB panel on the device: one chromosome-1-sized chain and the 22-chain genome, against one CPU core.

Workload: n = 1 244 783 (chr1 at 200 bp) and the 22 chain lengths of hg38 at 200 bp; bandwidth 32, Bartlett weights, B = 128
draws, z = 1.5, 2.0, 2.5, 3.0.  Device time is split into the host's noise stream (NumPy's generator), the upload
(csr_dwb_panel_begin), phase A (draws + order statistics) and phase B (draws again + tail statistics); kernel times come from the
library's profiler.  CPU: scripts/ubench/dwb_cpu.c, this project's plain-C restatement of ONE draw on one core, scaled to the
panel (2 B draws; the quantile and tail passes of the reference are not in that figure, so it is a lower bound of the CPU cost).
Prints one JSON line; --out writes it to a file too.

    python scripts/dwb_bench.py [--draws 128] [--scale 1] [--genome-group 0] [--no-genome] [--out profiles/dwb_bench.json]
"""
import argparse, ctypes as C, json, os, subprocess, sys, tempfile, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R)
import numpy as np

Z = (1.5, 2.0, 2.5, 3.0)
TQ = (0.9331927987311419, 0.9772498680518208, 0.9937903346742238, 0.9986501019683699)    # 1 - norm.sf(z)


def cpu_port():
    src = os.path.join(R, "scripts", "ubench", "dwb_cpu.c")
    so = os.path.join(tempfile.mkdtemp(prefix="dwb_cpu_"), "libdwb_cpu.so")
    subprocess.check_call(["gcc", "-O3", "-fno-trapping-math", "-fno-math-errno", "-mtune=generic", "-ffp-contract=off", "-shared",
                           "-fPIC", "-o", so, src, "-lm"])
    lib = C.CDLL(so)
    DP = C.POINTER(C.c_double)
    lib.dwb_draw_bartlett.argtypes = [DP, C.c_int64, C.c_int, DP, DP]

    def run(tmpl, bw, noise):
        out = np.empty(tmpl.size)
        assert lib.dwb_draw_bartlett(tmpl.ctypes.data_as(DP), tmpl.size, bw, noise.ctypes.data_as(DP), out.ctypes.data_as(DP)) == 0
        return out
    return run


def panel(lens, B, bw, group, label):
    """one panel through the C ABI, phase by phase"""
    from consenrich_amd import _lib as L, dwb
    lib = L.lib()
    rng = np.random.default_rng(1)
    tmpl = [rng.normal(0.0, 1.0, n) for n in lens]
    stride = max(lens) + 2 * dwb.max_lag(bw)
    t = time.perf_counter(); noise = dwb.noise_stream(0, B * stride); t_noise = time.perf_counter() - t
    nc, nz = len(lens), len(Z)
    n_arr, bw_arr, t_all = np.asarray(lens, np.int64), np.full(nc, bw, np.int32), np.concatenate(tmpl)
    ranks = np.array([[r for q in TQ for r in dwb.quantile_ranks(n, q)[:2]] for n in lens], np.int64)
    os_, cnt, soft = np.empty((nc, B, 2 * nz)), np.empty((nc, B, nz), np.int64), np.empty((nc, B, nz))
    L.check(lib.csr_profile_enable(None, 1))
    t = time.perf_counter()
    L.check_value(lib.csr_dwb_panel_begin(None, nc, n_arr.ctypes.data_as(L.I64P), bw_arr.ctypes.data_as(C.POINTER(C.c_int32)), b"bartlett",
                                          L.dp(t_all), L.dp(noise), noise.size, B, group))
    t_up = time.perf_counter() - t
    t = time.perf_counter(); L.check_value(lib.csr_dwb_panel_order_stats(None, 2 * nz, ranks.ctypes.data_as(L.I64P), L.dp(os_))); t_a = time.perf_counter() - t
    off = np.ascontiguousarray(np.quantile(os_[:, :, 1::2], 0.9, axis=1)); sc = np.ones((nc, nz))
    t = time.perf_counter(); L.check_value(lib.csr_dwb_panel_tail_stats(None, nz, L.dp(off), L.dp(sc), cnt.ctypes.data_as(L.I64P), L.dp(soft))); t_b = time.perf_counter() - t
    kt = (L.KernelTime * 64)(); nk = C.c_int32(0)
    L.check(lib.csr_profile_read(None, kt, 64, C.byref(nk)))
    kernels = {kt[i].name.decode(): round(kt[i].total_ms, 2) for i in range(min(nk.value, 64)) if kt[i].name.decode().startswith("dwb_")}
    L.check(lib.csr_profile_enable(None, 0))
    L.check(lib.csr_dwb_panel_end(None))
    total = t_noise + t_up + t_a + t_b
    return {"panel": label, "chains": nc, "bins": int(sum(lens)), "longest_chain": int(max(lens)), "draws": B, "bandwidth": bw,
            "draws_per_group": group, "noise_values": int(noise.size), "host_noise_ms": round(t_noise * 1e3, 1),
            "upload_ms": round(t_up * 1e3, 1), "phase_a_ms": round(t_a * 1e3, 1), "phase_b_ms": round(t_b * 1e3, 1),
            "total_ms": round(total * 1e3, 1), "host_noise_share": round(t_noise / total, 3), "kernel_ms": kernels,
            "mean_null_occupancy": float(np.mean(cnt[0, :, 0]) / lens[0])}, (tmpl[0], noise[:lens[0] + 2 * bw], os_[0, 0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=128)
    ap.add_argument("--bandwidth", type=int, default=32)
    ap.add_argument("--scale", type=int, default=1, help="divide every chain length by this (quick runs)")
    ap.add_argument("--genome-group", type=int, default=0, help="draws per group of the genome panel (0 = the library's default)")
    ap.add_argument("--no-genome", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from consenrich_amd.sharding import hg38_chain_lengths
    lens = [max(1, n // a.scale) for n in hg38_chain_lengths(200)]
    row = {"row": "stationary-null DWB panel, hg38 @200bp", "z": list(Z), "host_cores": os.cpu_count(), "cpu_cores_used": 1, "panels": []}
    panel([4096], 8, a.bandwidth, 0, "warm-up")
    chr1, (tmpl, noise, os0) = panel([max(lens)], a.draws, a.bandwidth, 0, "chr1")
    row["panels"].append(chr1)
    if not a.no_genome:
        genome, _ = panel(lens, a.draws, a.bandwidth, a.genome_group, "genome")
        row["panels"].append(genome)
        row["genome_over_chr1"] = round(genome["total_ms"] / chr1["total_ms"], 2)
        row["genome_over_chr1_device_only"] = round((genome["phase_a_ms"] + genome["phase_b_ms"]) / (chr1["phase_a_ms"] + chr1["phase_b_ms"]), 2)
    cpu = cpu_port()
    cpu(tmpl, a.bandwidth, noise)
    t = time.perf_counter(); d = cpu(tmpl, a.bandwidth, noise); t_c = time.perf_counter() - t
    srt = np.sort(d)
    from consenrich_amd import dwb
    want = np.array([srt[r] for q in TQ for r in dwb.quantile_ranks(d.size, q)[:2]])
    row["cpu"] = {"one_draw_ms": round(t_c * 1e3, 1), "bins": int(d.size), "panel_2B_draws_ms": round(2 * a.draws * t_c * 1e3, 1),
                  "order_statistics_of_draw_0_bit_identical_to_gpu": bool(np.array_equal(want.view(np.uint64), os0.view(np.uint64)))}
    row["cpu_one_core_over_gpu_chr1"] = round(row["cpu"]["panel_2B_draws_ms"] / chr1["total_ms"], 2)
    line = json.dumps(row)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
