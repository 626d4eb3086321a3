"""Measure the DWB peak scoring of a batch (DeviceBatch.dwb_peak_scoring) against the route a caller had before it.

    python scripts/peakscore_bench.py                 # 1 x MI355X: chr1 alone and the 22 autosomes
    python scripts/peakscore_bench.py --chr1-only

Writes profiles/peakscore_bench.json (--out).  Workload as scripts/segments_bench.py builds it: hg38 autosomes at 200 bp, per
chain one synthetic score track and a template, R = 64 replay draws (bandwidth 8), 5 scales x 4 views, per-view cap 1000, total
cap 20 000; --peaks exported peaks per chain (random spans of 5..50 bins).

Two routes to the same answer, both timed with the host clock around whole calls (every call ends synchronised), after one
untimed warm-up of the new call on chr1:
  new     DeviceBatch.dwb_peak_scoring, --repeats times (every timing is recorded): observed candidates, peaks scored on the resident
          track, the replays into the pool on the device, merge on the host, p / q on the device;
  before  DeviceBatch.dwb_replay (rows fetched and composed on the host), DeviceBatch.download_scores, then the step-by-step
          pure-Python twin of the scoring (tests/twin_peakscore.py score_steps), once each.
The two results are compared field by field, bit for bit (`identical`)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

SCALES = (1, 4, 8, 16, 32)
Z = (1.5, 2.0, 2.5, 3.0)
VIEW_CAP, TOTAL_CAP, REPLAYS, BANDWIDTH, SEED = 1000, 20000, 64, 8, 11


def _peaks(rng, n, count):
    starts = np.sort(rng.choice(max(n - 64, 1), size=min(count, max(n - 64, 1)), replace=False)).astype(np.int64)
    return starts, starts + rng.integers(4, 50, starts.shape[0])


def workload(name, lens, args, warm):
    import twin_peakscore as T
    from consenrich_amd import peakscore as P
    from consenrich_amd.batch import DeviceBatch, ModelParams

    rng = np.random.default_rng(7)
    nc = len(lens)
    tmpls = [rng.normal(0.0, 1.0, n) for n in lens]
    scores = [rng.normal(0.0, 1.0, n) for n in lens]
    peaks = [_peaks(rng, n, args.peaks) for n in lens]
    views = [[dict(threshold_z=z, threshold=z, null_scale=1.0, null_center=0.0) for z in Z] for _ in lens]
    kw = dict(bandwidths=[BANDWIDTH] * nc, templates=tmpls, num_replay=args.replays, random_seed=SEED, scale_bins=SCALES,
              max_segments=TOTAL_CAP, max_segments_per_view=VIEW_CAP, draws_per_group=args.draws_per_group)
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), 1, lens)
        for c in range(nc):
            b.upload_scores(c, scores[c])
        if warm:
            b.dwb_peak_scoring(views[:nc], peaks=peaks, **kw)
        t_new = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            new = b.dwb_peak_scoring(views, peaks=peaks, **kw)
            t_new.append(time.perf_counter() - t0)
        pool_stats = P.last_pool_stats()
        t0 = time.perf_counter()
        rep = b.dwb_replay(tmpls, views, **{k: v for k, v in kw.items() if k != "templates"})
        t_replay = time.perf_counter() - t0
        t0 = time.perf_counter()
        tracks = [b.download_scores(c) for c in range(nc)]
        t_download = time.perf_counter() - t0
    as_lists = [[(r, r["diagnostics"]) for r in rep[c]["replays"]] for c in range(nc)]
    per_chain, identical = [], True
    t_twin_total = 0.0
    for c in range(nc):
        spans = list(zip(peaks[c][0].tolist(), peaks[c][1].tolist()))
        vw = {str(i): v for i, v in enumerate(views[c])}
        t0 = time.perf_counter()
        want = T.score_steps(tracks[c], vw, rep[c]["observed"], as_lists[c], spans, scale_bins=rep[c]["scale_bins"],
                             dependence_span=BANDWIDTH, random_seed=SEED)
        t_twin = time.perf_counter() - t0
        t_twin_total += t_twin
        same = T.differences(new[c], want) == []
        identical = identical and same
        per_chain.append(dict(bins=int(lens[c]), peaks=len(spans), candidate_regions=len(want["candidate_details"]),
                              pooled_replay_candidates=int(sum(r["candidate_count"] for r in rep[c]["replays"])),
                              twin_scoring_seconds=t_twin, identical=bool(same)))
    before = t_replay + t_download + t_twin_total
    out = dict(chains=nc, bins=int(sum(lens)), replays=args.replays, scales=list(SCALES), views=len(Z), view_cap=VIEW_CAP,
               total_cap=TOTAL_CAP, peaks_per_chain=args.peaks, new_call_seconds=t_new, new_call_seconds_median=float(np.median(t_new)),
               replay_seconds=t_replay, download_scores_seconds=t_download, twin_scoring_seconds=t_twin_total,
               before_route_seconds=before, ratio_whole_route=before / float(np.median(t_new)), pool=pool_stats,
               identical=bool(identical), per_chain=per_chain)
    doc = {}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            doc = json.load(fh)
    doc[name] = out
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps({name: {k: v for k, v in out.items() if k != "per_chain"}}))
    return identical


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "peakscore_bench.json"))
    ap.add_argument("--replays", type=int, default=REPLAYS)
    ap.add_argument("--peaks", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--draws-per-group", type=int, default=0)
    ap.add_argument("--chr1-only", action="store_true")
    ap.add_argument("--bins", type=int, default=0, help="one chain of this many bins instead of the hg38 chains (a quick check)")
    args = ap.parse_args()
    from consenrich_amd import _lib as L
    from consenrich_amd.sharding import hg38_chain_lengths

    L.require_gpu()
    lens = [int(n) for n in hg38_chain_lengths(200)]
    if args.bins > 0:
        return 0 if workload(f"bins_{args.bins}", [args.bins], args, True) else 1
    ok = workload("chr1", lens[:1], args, True)
    if not args.chr1_only:
        ok = workload("genome_22_chains", lens, args, False) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
