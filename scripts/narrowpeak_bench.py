"""Measure the narrowPeak export of a fitted batch (DeviceBatch.narrowpeak_rows) against the route a caller had before it.

    python scripts/narrowpeak_bench.py                 # 1 x MI355X: chr1 alone and the 22 autosomes
    python scripts/narrowpeak_bench.py --chr1-only

Writes profiles/narrowpeak_bench.json (--out).  Workload: hg38 autosomes at 200 bp, one sample, the levelTrend fit of a synthetic
chain (tests/golden/cases.py `synth`); per chain a planted score track (parents of 1-4 Hann humps plus noise, 40..600 bins long,
joined by flat negative valleys; tests/nested_cases.py `planted`, as scripts/nested_bench.py plants them) whose parents are the
resident mask: --parents of them on chr1, --genome-parents over the 22 chains in proportion to their lengths.  gamma 1, selection
penalty 0.3, minSubpeakBins 5, trim floor 0, multiplier 2.

Two routes to the same answer, timed with the host clock around whole calls (every call ends synchronised), after one untimed
warm-up of the new call:
  new     DeviceBatch.narrowpeak_rows from the resident scores, masks and fit, --repeats times (every timing is recorded, with
          the library call's share and the host's share -- runs, gaps, assembly -- apart);
  before  the download of xs, Ps and the scores of every chain plus the reference-steps form of the pure-Python twin
          (tests/twin_narrowpeak.py `rows`), once.  The reference itself is not needed: the twin's steps form is held equal to it
          by the fixtures.
Rows, meta and details are compared bit for bit (`identical`)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

GAMMA, PENALTY, STEP = 1.0, 0.3, 200


def workload(name, lens, parents, args):
    import cases
    import twin_narrowpeak as T
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams
    from nested_bench import plant

    nc = len(lens)
    share = [max(1, int(round(parents * n / float(sum(lens))))) for n in lens]
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
        b.rocco(budget=0.1, gamma=GAMMA, selection_penalty=PENALTY)
        for c in range(nc):
            b.upload_solution(c, planted[c][1])
        t_new, t_dev = [], []
        for rep in range(args.repeats + 1):         # the first one is the warm-up
            t0 = time.perf_counter()
            new = b.narrowpeak_rows(PENALTY, GAMMA, interval_bp=STEP, chroms=names, prefix="bench")
            if rep:
                t_new.append(time.perf_counter() - t0)
                t_dev.append(float(b.narrowpeak_stats["device_seconds"]))
        stats = dict(b.narrowpeak_stats)
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
        want = T.rows(names[c], iv, iv + STEP, x, s, planted[c][1], "bench", 0.5, uncertainty=u, trimScoreFloor=0.0,
                      subpeakSelectionPenalty=PENALTY, subpeakBoundaryCost=0.25 * GAMMA, minSubpeakBins=5, returnExportDetails=True,
                      form="steps")
        t_twin = time.perf_counter() - t0
        t_twin_total += t_twin
        got = (new[c]["rows"], new[c]["peak_meta"], new[c]["export_details"])
        same = T.differences(got, want) == []
        identical = identical and same
        d = want[2]
        per_chain.append(dict(bins=int(lens[c]), selected_bins=int(planted[c][1].sum()), candidates=int(d["num_candidate_segments"]),
                              kept=int(d["num_segments_kept"]), dropped_median=int(d["num_segments_dropped_median_signal_local_p"]),
                              dropped_min_bp=int(d["num_segments_dropped_min_peak_bp"]), twin_seconds=t_twin, identical=bool(same)))
        print(f"{name}: chain {c} twin {t_twin:.1f} s identical {same}", flush=True)
    before = t_download + t_twin_total
    med = float(np.median(t_new))
    out = dict(chains=nc, bins=int(sum(lens)), parents=int(stats["parents"]), peaks=int(stats["peaks"]),
               decided_on_host=int(stats["decided_on_host"]), gamma=GAMMA, selection_penalty=PENALTY, min_subpeak_bins=5,
               new_call_seconds=t_new, new_call_seconds_median=med, device_call_seconds=t_dev,
               device_call_seconds_median=float(np.median(t_dev)), host_share_seconds_median=med - float(np.median(t_dev)),
               download_tracks_seconds=t_download, twin_seconds=t_twin_total, before_route_seconds=before,
               ratio_whole_route=before / med, identical=bool(identical), per_chain=per_chain)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "narrowpeak_bench.json"))
    ap.add_argument("--parents", type=int, default=3000, help="planted parents on chr1")
    ap.add_argument("--genome-parents", type=int, default=34000, help="planted parents over the 22 autosomes")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--chr1-only", action="store_true")
    ap.add_argument("--bins", type=int, default=0, help="one chain of this many bins instead of the hg38 chains (a quick check)")
    args = ap.parse_args()
    from consenrich_amd import _lib as L
    from consenrich_amd.sharding import hg38_chain_lengths

    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    L.require_gpu()
    lens = [int(n) for n in hg38_chain_lengths(200)]
    if args.bins > 0:
        return 0 if workload(f"bins_{args.bins}", [args.bins], args.parents, args) else 1
    ok = workload("chr1", lens[:1], args.parents, args)
    if not args.chr1_only:
        ok = workload("genome_22_chains", lens, args.genome_parents, args) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
