"""Measure the multiscale candidate-segment stage (csrc/csr_segments.h) against one CPU core.

    python scripts/segments_bench.py --cpu-check        # no GPU: the one-core C port against the compiled reference
    python scripts/segments_bench.py --device           # 1 x MI355X: device time per stage, chr1 alone and the 22-chain genome

Both write their section of profiles/segments_bench.json (--out) and leave the other one as it is.

--cpu-check (where `make -C oracle ref` has built the reference): scripts/ubench/segments_cpu.c, compiled with the reference's
flags, must equal the compiled `cMultiscaleCandidateSegmentStats` bit for bit on every case of tests/golden/segments_cases.py
(the per-view cap applied here with the reference's two NumPy calls); then both are timed on one track of --cpu-bins bins at
5 scales x 4 views.

--device: hg38 autosomes at 200 bp; per chain one observed track and R = 64 replay draws of the DWB panel (bandwidth 8), 5 scales
x 4 views, per-view cap 1000.  The replays go through csr_dwb_panel_begin / csr_dwb_panel_segments / csr_segments_fetch in groups
of draws sized to 16 GiB by the bound of include/consenrich_amd.h, the observed tracks through csr_segments_run; stage times are
the library's own event timers (csr_profile_read).  The CPU column is the C port on the observed track of every chain, times 65
tracks (measured once per chain, not 65 times)."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

UBENCH = os.path.join(ROOT, "scripts", "ubench")
PORT_SRC = os.path.join(UBENCH, "segments_cpu.c")
PORT_LIB = os.path.join(UBENCH, "libsegments_cpu.so")
REF_FLAGS = ["-O3", "-fno-trapping-math", "-fno-math-errno", "-mtune=generic", "-ffp-contract=off"]
SCALES = (1, 4, 8, 16, 32)
Z = (1.5, 2.0, 2.5, 3.0)
CAP, REPLAYS, BANDWIDTH = 1000, 64, 8
I64P, DP = C.POINTER(C.c_int64), C.POINTER(C.c_double)


def port():
    if not os.path.exists(PORT_LIB) or os.path.getmtime(PORT_LIB) < os.path.getmtime(PORT_SRC):
        subprocess.check_call(["gcc", *REF_FLAGS, "-shared", "-fPIC", "-o", PORT_LIB, PORT_SRC, "-lm"])
    lib = C.CDLL(PORT_LIB)
    lib.segments_cpu.restype = C.c_int64
    lib.segments_cpu.argtypes = [DP, C.c_int64, I64P, C.c_int32, DP, DP, C.c_int32, C.c_int32, C.c_int32, C.c_int64, I64P, I64P, DP,
                                 DP, DP, DP, I64P]
    return lib


def port_rows(lib, x, scales, thr, ns, min_run, gap, capacity=None):
    """The port's uncapped candidates: (start, end, score, integrated, mean, max), per-view counts, seconds of the C call."""
    x, thr, ns = (np.ascontiguousarray(a, np.float64) for a in (x, thr, ns))
    scales = np.ascontiguousarray(scales, np.int64)
    cap = int(capacity if capacity is not None else max(4 * x.shape[0], 1024))
    while True:
        ints = [np.empty(cap, np.int64) for _ in range(2)]
        flts = [np.empty(cap, np.float64) for _ in range(4)]
        counts = np.zeros(max(scales.shape[0] * thr.shape[0], 1), np.int64)
        t0 = time.perf_counter()
        rows = lib.segments_cpu(x.ctypes.data_as(DP), x.shape[0], scales.ctypes.data_as(I64P), scales.shape[0], thr.ctypes.data_as(DP),
                                ns.ctypes.data_as(DP), thr.shape[0], min_run, gap, cap, *[a.ctypes.data_as(I64P) for a in ints],
                                *[a.ctypes.data_as(DP) for a in flts], counts.ctypes.data_as(I64P))
        dt = time.perf_counter() - t0
        if rows < 0:
            raise MemoryError("segments_cpu")
        if rows <= cap:
            return [a[:rows] for a in ints + flts], counts, dt
        cap = int(rows)


def port_native(lib, x, scales, thr, ns, min_run=1, gap=0, cap=0):
    """The native's 11-tuple from the port's candidates (the cap: pyx:9629-9635's two NumPy calls)."""
    x = np.asarray(x, np.float64).reshape(-1)
    scales, thr, ns = np.asarray(scales, np.int64).reshape(-1), np.asarray(thr, np.float64), np.asarray(ns, np.float64)
    n = x.shape[0]
    if n == 0 or scales.shape[0] == 0 or thr.shape[0] == 0:
        return (*[np.zeros(0, np.int64)] * 4, *[np.zeros(0, np.float64)] * 4, 0, 0, 0)
    (st, en, score, integ, mean, mx), counts, _ = port_rows(lib, x, scales, thr, ns, min_run, gap)
    cap = max(cap, 0)
    cols, lo, hits, dropped = [[] for _ in range(8)], 0, 0, 0
    for si, w0 in enumerate(scales):
        w = int(min(max(int(w0), 1), n))
        for v in range(thr.shape[0]):
            k = int(counts[si * thr.shape[0] + v])
            sel = np.arange(lo, lo + k)
            if cap > 0 and k > cap:
                hits += 1
                dropped += k - cap
                part = np.argpartition(-score[lo:lo + k], cap - 1)[:cap]
                sel = lo + part[np.argsort(st[lo + part], kind="mergesort")]
            for col, val in zip(cols, (st[sel], en[sel], np.full(sel.shape[0], w, np.int64), np.full(sel.shape[0], v, np.int64),
                                       score[sel], integ[sel], mean[sel], mx[sel])):
                col.append(val)
            lo += k
    out = [np.concatenate(c).astype(np.int64 if q < 4 else np.float64) for q, c in enumerate(cols)]
    return (*out, int(counts.sum()), hits, dropped)


def _update(path, key, value):
    doc = {}
    if os.path.exists(path):
        with open(path) as fh:
            doc = json.load(fh)
    doc[key] = value
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps({key: value}))


def views():
    return np.asarray(Z, np.float64), np.ones(len(Z), np.float64)


def cpu_check(args):
    import segments_cases as SC
    import twin_segments as T
    from oracle import ref_loader

    ref = ref_loader.load()
    if ref is None:
        print("the compiled reference is not available (make -C oracle ref)", file=sys.stderr)
        return 2
    lib = port()

    class Port:
        @staticmethod
        def cMultiscaleCandidateSegmentStats(x, sc, thr, ns, min_run, gap, cap):
            return port_native(lib, x, sc, thr, ns, min_run, gap, cap)

    bad = [c["name"] for c in SC.cases() if not T.same(SC.run_case(ref, c), SC.run_case(Port, c))]
    print(f"{len(SC.cases())} cases, {len(bad)} differences between the C port and the compiled reference", bad)
    if bad:
        return 1
    x = np.random.default_rng(1).normal(0.0, 1.0, args.cpu_bins)
    thr, ns = views()
    sc = np.asarray(SCALES, np.int64)
    t_port = min(port_rows(lib, x, sc, thr, ns, 1, 0)[2] for _ in range(3))
    t_ref = []
    for _ in range(3):
        t0 = time.perf_counter()
        want = ref.cMultiscaleCandidateSegmentStats(x, sc, thr, ns, 1, 0, CAP)
        t_ref.append(time.perf_counter() - t0)
    same = T.same(want, port_native(lib, x, sc, thr, ns, 1, 0, CAP))
    _update(args.out, "cpu_port", dict(
        cases=len(SC.cases()), differences_from_compiled_reference=len(bad), timed_track_identical=bool(same), bins=args.cpu_bins,
        scales=list(SCALES), views=len(Z), cap=CAP, port_seconds=t_port, compiled_reference_seconds=min(t_ref),
        note="one core, best of 3; the port returns every candidate, the native also builds Python lists of its rows"))
    return 0 if same else 1


def _kernel_times(lib, L):
    buf = (L.KernelTime * 64)()
    n = C.c_int32()
    L.check(lib.csr_profile_read(None, buf, 64, C.byref(n)))
    return {buf[i].name.decode(): dict(launches=int(buf[i].launches), ms=float(buf[i].total_ms)) for i in range(min(n.value, 64))}


def device_workload(name, lens, args):
    from consenrich_amd import _lib as L
    from consenrich_amd import dwb, segments as S

    lib = L.lib()
    nc, R = len(lens), args.replays
    rng = np.random.default_rng(7)
    tmpls = [rng.normal(0.0, 1.0, n) for n in lens]
    observed = [rng.normal(0.0, 1.0, n) for n in lens]
    thr, ns = views()
    sc = [S.resolve_scales(n, SCALES) for n in lens]
    stride = max(lens) + 2 * dwb.max_lag(BANDWIDTH)
    noise = dwb.noise_stream(11, R * stride)
    group = dwb._replay_group(lens, [len(s) for s in sc], [len(Z)] * nc, R, args.draws_per_group)
    n_s, sc_all, n_v, thr_all, ns_all = S.pack(sc, [thr] * nc, [ns] * nc)
    n_arr, bw_arr = np.asarray(lens, np.int64), np.full(nc, BANDWIDTH, np.int32)
    t_all = np.ascontiguousarray(np.concatenate(tmpls))
    L.check(lib.csr_profile_enable(None, 1))
    rows_total = capped = flagged_total = 0
    t0 = time.perf_counter()
    L.check_value(lib.csr_dwb_panel_begin(None, nc, n_arr.ctypes.data_as(L.I64P), bw_arr.ctypes.data_as(L.I32P), b"bartlett", L.dp(t_all),
                                          L.dp(noise), noise.shape[0], R, group))
    t_begin = time.perf_counter() - t0
    t_collect = 0.0
    try:
        for d0 in range(0, R, group):
            g = min(group, R - d0)
            rows, counters, fl = np.zeros(nc * g, np.int64), np.zeros(3 * nc * g, np.int64), C.c_int32(0)
            L.check_value(lib.csr_dwb_panel_segments(None, d0, g, n_s.ctypes.data_as(L.I32P), sc_all.ctypes.data_as(L.I64P),
                                                     n_v.ctypes.data_as(L.I32P), L.dp(thr_all), L.dp(ns_all), 1, 0, CAP,
                                                     rows.ctypes.data_as(L.I64P), counters.ctypes.data_as(L.I64P), C.byref(fl)))
            t1 = time.perf_counter()
            S.collect(None, rows, counters, fl.value, CAP)
            t_collect += time.perf_counter() - t1
            rows_total += int(rows.sum())
            capped += S.last_run_stats()["capped_views"]
            flagged_total += fl.value
    finally:
        L.check(lib.csr_dwb_panel_end(None))
    t_replays = time.perf_counter() - t0
    t0 = time.perf_counter()
    for c in range(nc):
        S.cMultiscaleCandidateSegmentStats(observed[c], sc[c], thr, ns, 1, 0, CAP)
    t_observed = time.perf_counter() - t0
    times = _kernel_times(lib, L)
    L.check(lib.csr_profile_enable(None, 0))
    cpu = None
    if not args.no_cpu:
        plib = port()
        cpu = sum(port_rows(plib, observed[c], sc[c], thr, ns, 1, 0)[2] for c in range(nc))
    seg = {k: v for k, v in times.items() if k.startswith("seg_")}
    out = dict(chains=nc, bins=int(sum(lens)), replays=R, draws_per_group=group, scales=list(SCALES), views=len(Z), cap=CAP,
               wall_seconds_replays=t_replays, wall_seconds_panel_begin_upload=t_begin, wall_seconds_resolve_and_fetch=t_collect,
               wall_seconds_observed_tracks=t_observed, rows=rows_total, capped_views=capped, fallback_views=flagged_total,
               device_ms=dict(sorted(times.items())), device_ms_segments_total=sum(v["ms"] for v in seg.values()),
               cpu_port_seconds_one_track_per_chain=cpu, cpu_port_seconds_65_tracks=None if cpu is None else 65.0 * cpu)
    _update(args.out, name, out)


def device(args):
    from consenrich_amd import _lib as L
    from consenrich_amd.sharding import hg38_chain_lengths

    L.require_gpu()
    lens = [int(n) for n in hg38_chain_lengths(200)]
    device_workload("chr1", lens[:1], args)
    if not args.chr1_only:
        device_workload("genome_22_chains", lens, args)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cpu-check", action="store_true")
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segments_bench.json"))
    ap.add_argument("--cpu-bins", type=int, default=1_244_783, help="bins of the timed CPU track (chr1 at 200 bp)")
    ap.add_argument("--replays", type=int, default=REPLAYS)
    ap.add_argument("--draws-per-group", type=int, default=0)
    ap.add_argument("--chr1-only", action="store_true")
    ap.add_argument("--no-cpu", action="store_true", help="--device: skip the CPU column")
    args = ap.parse_args()
    if not (args.cpu_check or args.device):
        ap.error("one of --cpu-check / --device")
    rc = cpu_check(args) if args.cpu_check else 0
    if rc == 0 and args.device:
        rc = device(args)
    return rc


if __name__ == "__main__":
    sys.exit(main())
