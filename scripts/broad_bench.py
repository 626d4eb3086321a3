"""Measure broad mode's bridging and rows of a fitted batch (DeviceBatch.broad_parents + DeviceBatch.broadpeak_rows) against the
route a caller had before them.

    python scripts/broad_bench.py                 # 1 x MI355X: chr1 alone and the 22 autosomes
    python scripts/broad_bench.py --chr1-only

Writes profiles/broad_bench.json (--out).  Workload: hg38 autosomes at 200 bp, one sample, the levelTrend fit of a synthetic chain
(tests/golden/cases.py `synth`); per chain a planted score track: noise about -0.5, and --domains (chr1) or --genome-domains (the
22 chains, in proportion to their lengths) broad domains of 400..6000 bins, each a row of plateaus of 80..400 bins at 1.2 with dips
of 2..12 bins at -0.1 between them.  The strong mask holds the middle 20 bins of every third plateau, the weak mask four plateaus
of five whole.  Support threshold 0.5, selection penalty 0.2, boundary cost 1.0, dip fraction 0.5, maxGapBP 4 * 3 * 200.

Two routes to the same answer, timed with the host clock around whole calls (every call ends synchronised), after one untimed
warm-up of the new calls:
  new     broad_parents + broadpeak_rows from the resident scores, masks and fit, --repeats times; the median is reported, with the
          library calls' share (the run call with its fetch, and the rows call) and the host's Python apart;
  before  the download of xs, Ps and the scores of every chain plus the reference-steps form of the pure-Python twin
          (tests/twin_broad.py `parents` and `rows`), once.  The reference itself is not needed: the twin's steps form is held
          equal to it by the fixtures.
Merged runs, details, rows and meta are compared bit for bit (`identical`)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

THRESHOLD, PENALTY, COST, STEP, MAX_GAP = 0.5, 0.2, 1.0, 200, 4 * 3 * 200


def plant(seed, n, domains):
    """(scores, strong mask, weak mask) of one chain"""
    rng = np.random.default_rng(seed)
    s = -0.5 + 0.3 * rng.standard_normal(n)
    strong, weak = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    slot = n // max(domains, 1)
    k = 0
    for d in range(domains):
        length = int(rng.integers(400, 6001))
        pos = d * slot + int(rng.integers(0, max(slot - length, 1)))
        end = min(pos + length, (d + 1) * slot - 20, n - 1)
        while pos < end:
            width = min(int(rng.integers(80, 401)), end - pos)
            s[pos:pos + width] = 1.2 + 0.2 * rng.standard_normal(width)
            if k % 3 == 0 and width > 40:
                strong[pos + width // 2 - 10:pos + width // 2 + 10] = 1
            if k % 5 != 4:
                weak[pos:pos + width] = 1
            k += 1
            pos += width
            dip = min(int(rng.integers(2, 13)), max(end - pos, 0))
            s[pos:pos + dip] = -0.1 + 0.1 * rng.standard_normal(dip)
            pos += dip
    s = np.where(np.abs(s - THRESHOLD) < 1e-6, THRESHOLD + 0.01, s)
    return s, strong, weak


def workload(name, lens, domains, args):
    import broad_cases as BC
    import cases
    import twin_broad as T
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    nc = len(lens)
    share = [max(1, int(round(domains * n / float(sum(lens))))) for n in lens]
    planted = [plant(100 + c, lens[c], share[c]) for c in range(nc)]
    names = [f"chr{c + 1}" for c in range(nc)]
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), 1, lens)
        for c in range(nc):
            b.upload(c, *cases.synth(lens[c], 1, 300 + c))
        b.stats()
        b.forward_backward(L.RETURN_NLL)
        b.export(L.EXPORT_SMOOTH)
        for c in range(nc):
            b.upload_scores(c, planted[c][0])
        b.rocco(budget=0.1, gamma=COST, selection_penalty=PENALTY)
        for c in range(nc):
            b.upload_solution(c, planted[c][1])
            b.upload_weak_solution(c, planted[c][2])
        t_new, t_lib, t_runs, t_rows = [], [], [], []
        for rep in range(args.repeats + 1):         # the first one is the warm-up
            t0 = time.perf_counter()
            par = b.broad_parents(THRESHOLD, PENALTY, COST, max_gap_bp=MAX_GAP, interval_bp=STEP, chroms=names)
            new = b.broadpeak_rows(interval_bp=STEP, chroms=names, prefix="bench")
            if rep:
                t_new.append(time.perf_counter() - t0)
                t_runs.append(float(b.broad_stats["device_seconds"]))
                t_rows.append(float(b.broad_stats["rows_device_seconds"]))
                t_lib.append(t_runs[-1] + t_rows[-1])
        stats = dict(b.broad_stats)
        t0 = time.perf_counter()
        tracks = []
        for c in range(nc):
            x = b.download(c, "xs")[:, 0].astype(np.float64)
            u = np.sqrt(b.download(c, "Ps")[:, 0, 0]).astype(np.float64)
            tracks.append((x, u, b.download_scores(c)))
        t_download = time.perf_counter() - t0
    per_chain, identical, t_twin_total = [], True, 0.0
    for c in range(nc):
        iv = np.arange(lens[c], dtype=np.int64) * STEP
        x, u, s = tracks[c]
        t0 = time.perf_counter()
        wp = T.parents(s, planted[c][1], planted[c][2], THRESHOLD, iv, iv + STEP, names[c], PENALTY, COST, MAX_GAP)
        wr = T.rows(names[c], iv, iv + STEP, x, s, wp["mask"], planted[c][1], "bench", uncertainty=u, returnExportDetails=True)
        t_twin = time.perf_counter() - t0
        t_twin_total += t_twin
        g, r = par[c], new[c]
        same = (g["starts"].tolist(), g["ends"].tolist()) == (wp["starts"], wp["ends"]) and \
            BC.canon(g["merge_details"]) == BC.canon(wp["merge_details"]) and \
            BC.canon((r["broad_rows"], r["gapped_rows"], r["peak_meta"], r["export_details"])) == BC.canon(wr)
        identical = identical and same
        d, md = wr[3], wp["merge_details"]
        widths = [m["end_idx"] - m["start_idx"] + 1 for m in wr[2]]
        per_chain.append(dict(bins=int(lens[c]), support_runs=int(wp["weak_support_run_count"]),
                              touching_runs=int(wp["weak_support_touching_run_count"]), gaps_merged=int(md.get("num_gaps_merged", 0)),
                              parents=int(d["num_candidate_segments"]), kept=int(d["num_segments_kept"]),
                              median_parent_bins=float(np.median(widths)) if widths else 0.0,
                              longest_parent_bins=int(max(widths)) if widths else 0, twin_seconds=t_twin, identical=bool(same)))
        print(f"{name}: chain {c} twin {t_twin:.1f} s identical {same}", flush=True)
    before = t_download + t_twin_total
    med, lib = float(np.median(t_new)), float(np.median(t_lib))
    out = dict(chains=nc, bins=int(sum(lens)), support_runs=int(stats["support_runs"]), kept_runs=int(stats["kept_runs"]),
               parents=int(stats["row_parents"]), rows=int(stats["rows"]), decided_on_host=int(stats["decided_on_host"]),
               threshold=THRESHOLD, selection_penalty=PENALTY, boundary_cost=COST, max_gap_bp=MAX_GAP,
               new_route_seconds=t_new, new_route_seconds_median=med, library_calls_seconds=t_lib, library_calls_seconds_median=lib,
               runs_call_seconds_median=float(np.median(t_runs)), rows_call_seconds_median=float(np.median(t_rows)),
               host_python_seconds_median=med - lib, download_tracks_seconds=t_download, twin_seconds=t_twin_total,
               before_route_seconds=before, ratio_whole_route=before / med, identical=bool(identical), per_chain=per_chain)
    doc = {}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            doc = json.load(fh)
    doc[name] = out
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps({name: {k: v for k, v in out.items() if k != "per_chain"}}), flush=True)
    return identical


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "broad_bench.json"))
    ap.add_argument("--domains", type=int, default=120, help="planted domains on chr1")
    ap.add_argument("--genome-domains", type=int, default=1400, help="planted domains over the 22 autosomes")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--chr1-only", action="store_true")
    ap.add_argument("--bins", type=int, default=0, help="one chain of this many bins instead of the hg38 chains (a quick check)")
    args = ap.parse_args()
    from consenrich_amd import _lib as L
    from consenrich_amd.sharding import hg38_chain_lengths

    L.require_gpu()
    lens = [int(n) for n in hg38_chain_lengths(200)]
    if args.bins > 0:
        return 0 if workload(f"bins_{args.bins}", [args.bins], args.domains, args) else 1
    ok = workload("chr1", lens[:1], args.domains, args)
    if not args.chr1_only:
        ok = workload("genome_22_chains", lens, args.genome_domains, args) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
