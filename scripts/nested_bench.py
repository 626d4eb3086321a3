"""Measure the nested ROCCO refinement of a batch (DeviceBatch.rocco_nested) against the route a caller had before it.

    python scripts/nested_bench.py                 # 1 x MI355X: chr1 alone and the 22 autosomes
    python scripts/nested_bench.py --chr1-only

Writes profiles/nested_bench.json (--out).  Workload: hg38 autosomes at 200 bp; per chain a planted score track (parents of 1-4
Hann humps plus noise, 40..600 bins long, joined by flat negative valleys of 1..40 bins; tests/nested_cases.py `planted`) whose
parents are the first-pass mask: --parents of them on chr1, --genome-parents over the 22 chains in proportion to their lengths.
gamma 1, selection penalty 0.3, three layers, budget scale 0.75, bin mode.

Two routes to the same answer, timed with the host clock around whole calls (every call ends synchronised), after one untimed
warm-up of the new call:
  new     DeviceBatch.rocco_nested from the resident scores and masks, --repeats times (every timing is recorded; the first-pass
          mask is uploaded again before each repeat, outside the timing);
  before  DeviceBatch.download_scores plus the reference-steps form of the pure-Python twin (tests/twin_nested.py `refine`), once.
          The reference itself is not needed: the twin's steps form is held equal to it by the fixtures.
Masks and details are compared bit for bit (`identical`)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

GAMMA, PENALTY = 1.0, 0.3


def plant(seed, n, parents):
    """(scores, mask) of n bins: as many planted parents as fit, at most `parents`; the rest of the chain is the valley level"""
    import nested_cases as NC

    rng = np.random.default_rng(seed)
    lengths = np.exp(rng.uniform(np.log(40), np.log(600), parents)).astype(int)
    keep = int(np.searchsorted(np.cumsum(lengths + 41), n - 8))
    x, sol = NC.planted(seed, lengths[:keep].tolist())
    scores, mask = np.full(n, -1.0), np.zeros(n, np.uint8)
    scores[:x.size], mask[:x.size] = x[:n], sol[:n]
    return scores, mask


def workload(name, lens, parents, args):
    import twin_nested as T
    from consenrich_amd.batch import DeviceBatch, ModelParams

    nc = len(lens)
    share = [max(1, int(round(parents * n / float(sum(lens))))) for n in lens]
    planted = [plant(100 + c, lens[c], share[c]) for c in range(nc)]
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), 1, lens)
        for c in range(nc):
            b.upload_scores(c, planted[c][0])
        b.rocco(budget=0.1, gamma=GAMMA, selection_penalty=PENALTY)
        t_new = []
        for rep in range(args.repeats + 1):         # the first one is the warm-up
            for c in range(nc):
                b.upload_solution(c, planted[c][1])
            t0 = time.perf_counter()
            new = b.rocco_nested(GAMMA, PENALTY)
            if rep:
                t_new.append(time.perf_counter() - t0)
        masks = [b.rocco_solution(c) for c in range(nc)]
        t0 = time.perf_counter()
        tracks = [b.download_scores(c) for c in range(nc)]
        t_download = time.perf_counter() - t0
    per_chain, identical, t_twin_total = [], True, 0.0
    for c in range(nc):
        t0 = time.perf_counter()
        want_mask, want = T.refine(tracks[c], planted[c][1], GAMMA, PENALTY, form="steps")
        t_twin = time.perf_counter() - t0
        t_twin_total += t_twin
        same = bool(np.array_equal(masks[c], want_mask)) and T.differences(new[c], want) == []
        identical = identical and same
        decisions = [n["decision"] for n in want["hierarchy"]]
        per_chain.append(dict(bins=int(lens[c]), parents=len(want["root_ids"]), selected_bins=int(want["initial_selected_count"]),
                              final_selected_bins=int(want["final_selected_count"]), nodes=len(decisions),
                              splits=decisions.count("split"), shrinks=decisions.count("shrink"), layers=int(want["completed_iters"]),
                              stop_reason=want["stop_reason"], twin_seconds=t_twin, identical=same))
        print(f"{name}: chain {c} twin {t_twin:.1f} s identical {same}", flush=True)
    before = t_download + t_twin_total
    out = dict(chains=nc, bins=int(sum(lens)), parents=int(sum(p["parents"] for p in per_chain)),
               selected_bins=int(sum(p["selected_bins"] for p in per_chain)), gamma=GAMMA, selection_penalty=PENALTY, layers=3,
               budget_scale=0.75, new_call_seconds=t_new, new_call_seconds_median=float(np.median(t_new)),
               download_scores_seconds=t_download, twin_seconds=t_twin_total, before_route_seconds=before,
               ratio_whole_route=before / float(np.median(t_new)), identical=bool(identical), per_chain=per_chain)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nested_bench.json"))
    ap.add_argument("--parents", type=int, default=3000, help="planted parents on chr1")
    ap.add_argument("--genome-parents", type=int, default=34000, help="planted parents over the 22 autosomes")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--chr1-only", action="store_true")
    ap.add_argument("--bins", type=int, default=0, help="one chain of this many bins instead of the hg38 chains (a quick check)")
    args = ap.parse_args()
    from consenrich_amd import _lib as L
    from consenrich_amd.sharding import hg38_chain_lengths

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
